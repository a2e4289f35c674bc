// hipblas{S,D,C,Z}trmm through the hook, with the program LINKED against libgemmul8.so in front of hipBLAS (INTEGRATION.md "link-time": no
// LD_PRELOAD anywhere): the hook's definitions of the hipBLAS names come first in the search order, the direct emulation is called by name.
//   emu          (GEMMUL8_NUM_MOD_* set by the caller): hipblasStrmm, hipblasDtrmm, hipblasDtrmm_64, hipblasCtrmm, hipblasZtrmm == gemmul8_trmm bit for bit
//                over the WHOLE sentinel-filled C buffer; the other triangle of A (and, under UNIT, its diagonal) holds NaN; one call in place (C == B)
//   exact s|d|c|z small-integer data, so the exact answer is known whichever routine -- native or emulated -- serves the call; the caller reads from the
//                stats line which one did
#include <hip/hip_runtime.h>
#include <hipblas/hipblas.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/gemmul8_c.h"

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                  \
        }                                                              \
    } while (0)

template <typename T> T* dev(const std::vector<T>& h) {
    T* d;
    hipMalloc(&d, h.size() * sizeof(T));
    hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    return d;
}
template <typename T> std::vector<T> host(const T* d, size_t count) {
    std::vector<T> h(count);
    hipDeviceSynchronize();
    hipMemcpy(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost);
    return h;
}
template <typename T> T sentinel() {
    T v;
    std::memset(&v, 0xA5, sizeof v);
    return v;
}
template <typename T> struct Ty;
template <> struct Ty<float> {
    using R = float;
    static constexpr int code = GEMMUL8_S, comps = 1;
    static constexpr const char* env = "GEMMUL8_NUM_MOD_S";
};
template <> struct Ty<double> {
    using R = double;
    static constexpr int code = GEMMUL8_D, comps = 1;
    static constexpr const char* env = "GEMMUL8_NUM_MOD_D";
};
template <> struct Ty<hipComplex> {
    using R = float;
    static constexpr int code = GEMMUL8_C, comps = 2;
    static constexpr const char* env = "GEMMUL8_NUM_MOD_C";
};
template <> struct Ty<hipDoubleComplex> {
    using R = double;
    static constexpr int code = GEMMUL8_Z, comps = 2;
    static constexpr const char* env = "GEMMUL8_NUM_MOD_Z";
};
template <typename T> T make(double re, double im) {
    typename Ty<T>::R p[2] = {(typename Ty<T>::R)re, (typename Ty<T>::R)im};
    T v;
    std::memcpy(&v, p, sizeof(T));
    return v;
}
template <typename T> double part(const T& v, int c) {
    typename Ty<T>::R p[2] = {0, 0};
    std::memcpy(p, &v, sizeof(T));
    return (double)p[c];
}
inline bool stored(hipblasFillMode_t uplo, int i, int j) { return uplo == HIPBLAS_FILL_MODE_LOWER ? i >= j : i <= j; }

#define OZ2_TRMM_CALLS(T, U)                                                                                                                        \
    inline hipblasStatus_t trmm(hipblasHandle_t h, hipblasSideMode_t s, hipblasFillMode_t u, hipblasOperation_t t, hipblasDiagType_t d, int m, int n, \
                                const T* al, const T* A, int lda, const T* B, int ldb, T* C, int ldc) {                                             \
        return hipblas##U##trmm(h, s, u, t, d, m, n, al, A, lda, B, ldb, C, ldc);                                                                   \
    }                                                                                                                                               \
    inline hipblasStatus_t trmm64(hipblasHandle_t h, hipblasSideMode_t s, hipblasFillMode_t u, hipblasOperation_t t, hipblasDiagType_t d, int m, int n, \
                                  const T* al, const T* A, int lda, const T* B, int ldb, T* C, int ldc) {                                           \
        return hipblas##U##trmm_64(h, s, u, t, d, (int64_t)m, (int64_t)n, al, A, (int64_t)lda, B, (int64_t)ldb, C, (int64_t)ldc);                   \
    }
OZ2_TRMM_CALLS(float, S)
OZ2_TRMM_CALLS(double, D)
OZ2_TRMM_CALLS(hipComplex, C)
OZ2_TRMM_CALLS(hipDoubleComplex, Z)

template <typename T>
int emulated(hipblasHandle_t handle, hipblasSideMode_t side, hipblasFillMode_t uplo, hipblasOperation_t trans, hipblasDiagType_t diag, bool ilp64, bool inplace) {
    const unsigned N = (unsigned)std::atoi(std::getenv(Ty<T>::env));
    const int m = 300, n = 200, ka = side == HIPBLAS_SIDE_LEFT ? m : n, lda = ka + 3, ldb = m + 1, ldc = inplace ? ldb : m + 7;
    std::mt19937 gen(3);
    std::uniform_real_distribution<double> U(-0.5, 0.5);
    const double nan = std::nan("");
    std::vector<T> hA((size_t)lda * ka, make<T>(nan, nan)), hB((size_t)ldb * n, sentinel<T>()), hC((size_t)ldc * n, sentinel<T>());
    for (int j = 0; j < ka; ++j)
        for (int i = 0; i < ka; ++i)
            if (stored(uplo, i, j) && !(i == j && diag == HIPBLAS_DIAG_UNIT)) hA[(size_t)j * lda + i] = make<T>(U(gen), U(gen));
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < m; ++i) hB[(size_t)j * ldb + i] = make<T>(8 * U(gen), 8 * U(gen));
    if (inplace) hC = hB;
    T *A = dev(hA), *B1 = dev(hB), *B2 = dev(hB), *C1 = inplace ? B1 : dev(hC), *C2 = inplace ? B2 : dev(hC);
    const T alpha = make<T>(0.75, Ty<T>::comps == 2 ? -0.25 : 0.0);
    void* work;
    hipMalloc(&work, gemmul8_work_size(Ty<T>::comps == 2, GEMMUL8_INT8, m, n, ka, N, 0, 0, nullptr, nullptr));  // the equivalent GEMM's
    CHECK(gemmul8_trmm(nullptr, Ty<T>::code, GEMMUL8_INT8, (int)side, (int)uplo, (int)trans, (int)diag, m, n, &alpha, A, lda, B2, ldb, C2, ldc, N, 0, work, nullptr) == 0);
    const hipblasStatus_t st = ilp64 ? trmm64(handle, side, uplo, trans, diag, m, n, &alpha, A, lda, B1, ldb, C1, ldc)
                                     : trmm(handle, side, uplo, trans, diag, m, n, &alpha, A, lda, B1, ldb, C1, ldc);
    CHECK(st == HIPBLAS_STATUS_SUCCESS);
    const std::vector<T> got = host(C1, hC.size()), ref = host(C2, hC.size());
    CHECK(std::memcmp(got.data(), ref.data(), got.size() * sizeof(T)) == 0);  // hooked == direct, bit for bit
    size_t changed = 0;
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < ldc; ++i) {
            const size_t e = (size_t)j * ldc + i;
            if (i >= m) CHECK(std::memcmp(&got[e], &hC[e], sizeof(T)) == 0);  // the ldc padding: untouched
            else {
                changed += std::memcmp(&got[e], &hC[e], sizeof(T)) != 0;
                for (int c = 0; c < Ty<T>::comps; ++c) CHECK(std::isfinite(part(got[e], c)));  // no NaN of A's unused parts came through
            }
        }
    CHECK(changed > (size_t)m * n - 8);
    hipFree(A), hipFree(B1), hipFree(B2), hipFree(work);
    if (!inplace) hipFree(C1), hipFree(C2);
    return 0;
}

// m = n = ka = 8, side = left, uplo = lower, op = N, non-unit: m n ka = 512
template <typename T> int exact(hipblasHandle_t handle) {
    const int n = 8, ldc = n + 3;
    std::mt19937 gen(4);
    auto small = [&] { return (double)((int)(gen() % 3) - 1); };  // -1, 0, 1: every sum is an exact small integer
    std::vector<T> hA((size_t)n * n), hB((size_t)n * n), hC((size_t)ldc * n, sentinel<T>());
    for (auto& x : hA) x = make<T>(small(), Ty<T>::comps == 2 ? small() : 0.0);
    for (auto& x : hB) x = make<T>(small(), Ty<T>::comps == 2 ? small() : 0.0);
    T *A = dev(hA), *B = dev(hB), *C = dev(hC);
    const T alpha = make<T>(2, 0);
    CHECK(trmm(handle, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, HIPBLAS_DIAG_NON_UNIT, n, n, &alpha, A, n, B, n, C, ldc) == HIPBLAS_STATUS_SUCCESS);
    const std::vector<T> got = host(C, hC.size());
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < ldc; ++i) {
            const size_t e = (size_t)j * ldc + i;
            if (i >= n) {
                CHECK(std::memcmp(&got[e], &hC[e], sizeof(T)) == 0);
                continue;
            }
            double sr = 0, si = 0;  // (Atri B)(i, j) from the lower triangle of A
            for (int l = 0; l <= i; ++l) {
                const T &a = hA[(size_t)l * n + i], &b = hB[(size_t)j * n + l];
                sr += part(a, 0) * part(b, 0) - part(a, 1) * part(b, 1);
                si += part(a, 0) * part(b, 1) + part(a, 1) * part(b, 0);
            }
            if (part(got[e], 0) != 2 * sr || (Ty<T>::comps == 2 && part(got[e], 1) != 2 * si))
                std::printf("type %d (%d, %d): got (%g, %g), exact (%g, %g)\n", Ty<T>::code, i, j, part(got[e], 0), part(got[e], 1), 2 * sr, 2 * si);
            CHECK(part(got[e], 0) == 2 * sr);
            if (Ty<T>::comps == 2) CHECK(part(got[e], 1) == 2 * si);
        }
    hipFree(A), hipFree(B), hipFree(C);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("FAILED: run me as `test_hook_trmm emu | exact [sdcz]`\n");
        return 1;
    }
    hipSetDevice(0);
    {  // what the allocator hands out next has been written before: nothing may depend on fresh memory being zero
        void* dirt;
        if (hipMalloc(&dirt, (size_t)1 << 30) == hipSuccess) {
            hipMemset(dirt, 0x5B, (size_t)1 << 30);
            hipDeviceSynchronize();
            hipFree(dirt);
        }
    }
    hipblasHandle_t handle;
    hipblasCreate(&handle);
    if (!std::strcmp(argv[1], "emu")) {
        if (emulated<float>(handle, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, HIPBLAS_DIAG_NON_UNIT, false, false)) return 1;
        if (emulated<double>(handle, HIPBLAS_SIDE_RIGHT, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_T, HIPBLAS_DIAG_UNIT, false, true)) return 1;
        if (emulated<double>(handle, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_N, HIPBLAS_DIAG_NON_UNIT, true, false)) return 1;
        if (emulated<hipComplex>(handle, HIPBLAS_SIDE_RIGHT, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_C, HIPBLAS_DIAG_NON_UNIT, false, false)) return 1;
        if (emulated<hipDoubleComplex>(handle, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_C, HIPBLAS_DIAG_UNIT, false, false)) return 1;
        std::printf("hooked hipblas{S,D,C,Z}trmm (+ Dtrmm_64, one in place) == direct gemmul8_trmm (bitwise), ldc padding untouched\n");
    } else {
        const char* which = argc > 2 ? argv[2] : "sdcz";
        if (std::strchr(which, 's') && exact<float>(handle)) return 1;
        if (std::strchr(which, 'd') && exact<double>(handle)) return 1;
        if (std::strchr(which, 'c') && exact<hipComplex>(handle)) return 1;
        if (std::strchr(which, 'z') && exact<hipDoubleComplex>(handle)) return 1;
        std::printf("hipblas?trmm (%s): exact small-integer result\n", which);
    }
    CHECK(hipblasDestroy(handle) == HIPBLAS_STATUS_SUCCESS);
    std::printf("ALL OK\n");
    return 0;
}
