// hipblas{S,D,C,Z}trsm through the hook, with the program LINKED against libgemmul8.so in front of hipBLAS (INTEGRATION.md "link-time": no
// LD_PRELOAD anywhere): the hook's definitions of the hipBLAS names come first in the search order, the direct emulation is called by name.
//   emu          (GEMMUL8_NUM_MOD_* set by the caller): hipblasStrsm, hipblasDtrsm, hipblasDtrsm_64, hipblasCtrsm, hipblasZtrsm == gemmul8_trsm bit for bit
//                over the WHOLE sentinel-padded B buffer (the call is in place on B); the other triangle of A (and, under UNIT, its diagonal) holds NaN
//   exact s|d|c|z data whose solution is a matrix of small integers and whose every intermediate is exact, so the answer is known whichever routine --
//                native or emulated -- serves the call; the caller reads from the stats line which one did
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

#define OZ2_TRSM_CALLS(T, U)                                                                                                                        \
    inline hipblasStatus_t trsm(hipblasHandle_t h, hipblasSideMode_t s, hipblasFillMode_t u, hipblasOperation_t t, hipblasDiagType_t d, int m, int n, \
                                const T* al, const T* A, int lda, T* B, int ldb) {                                                                  \
        return hipblas##U##trsm(h, s, u, t, d, m, n, al, A, lda, B, ldb);                                                                           \
    }                                                                                                                                               \
    inline hipblasStatus_t trsm64(hipblasHandle_t h, hipblasSideMode_t s, hipblasFillMode_t u, hipblasOperation_t t, hipblasDiagType_t d, int m, int n, \
                                  const T* al, const T* A, int lda, T* B, int ldb) {                                                                \
        return hipblas##U##trsm_64(h, s, u, t, d, (int64_t)m, (int64_t)n, al, A, (int64_t)lda, B, (int64_t)ldb);                                    \
    }
OZ2_TRSM_CALLS(float, S)
OZ2_TRSM_CALLS(double, D)
OZ2_TRSM_CALLS(hipComplex, C)
OZ2_TRSM_CALLS(hipDoubleComplex, Z)

template <typename T>
int emulated(hipblasHandle_t handle, hipblasSideMode_t side, hipblasFillMode_t uplo, hipblasOperation_t trans, hipblasDiagType_t diag, bool ilp64) {
    const unsigned N = (unsigned)std::atoi(std::getenv(Ty<T>::env));
    const int m = 300, n = 200, ka = side == HIPBLAS_SIDE_LEFT ? m : n, lda = ka + 3, ldb = m + 5;
    std::mt19937 gen(3);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    const double nan = std::nan("");
    std::vector<T> hA((size_t)lda * ka, make<T>(nan, nan)), hB((size_t)ldb * n, sentinel<T>());
    for (int j = 0; j < ka; ++j)   // well conditioned: off-diagonal entries within +-1/ka, diagonal magnitudes in [1, 2]
        for (int i = 0; i < ka; ++i) {
            if (!stored(uplo, i, j) || (i == j && diag == HIPBLAS_DIAG_UNIT)) continue;
            hA[(size_t)j * lda + i] = i == j ? make<T>((U(gen) < 0 ? -1 : 1) * (1.5 + 0.5 * U(gen)), 0.0) : make<T>(U(gen) / ka, Ty<T>::comps == 2 ? U(gen) / ka : 0.0);
        }
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < m; ++i) hB[(size_t)j * ldb + i] = make<T>(U(gen), Ty<T>::comps == 2 ? U(gen) : 0.0);
    T *A = dev(hA), *B1 = dev(hB), *B2 = dev(hB);
    const T alpha = make<T>(0.75, Ty<T>::comps == 2 ? -0.25 : 0.0);
    void* work;
    hipMalloc(&work, gemmul8_trsm_work_size(Ty<T>::comps == 2, GEMMUL8_INT8, (int)side, m, n, N));
    CHECK(gemmul8_trsm(nullptr, Ty<T>::code, GEMMUL8_INT8, (int)side, (int)uplo, (int)trans, (int)diag, m, n, &alpha, A, lda, B2, ldb, N, 0, work, nullptr) == 0);
    const hipblasStatus_t st = ilp64 ? trsm64(handle, side, uplo, trans, diag, m, n, &alpha, A, lda, B1, ldb) : trsm(handle, side, uplo, trans, diag, m, n, &alpha, A, lda, B1, ldb);
    CHECK(st == HIPBLAS_STATUS_SUCCESS);
    const std::vector<T> got = host(B1, hB.size()), ref = host(B2, hB.size());
    CHECK(std::memcmp(got.data(), ref.data(), got.size() * sizeof(T)) == 0);  // hooked == direct, bit for bit
    size_t changed = 0;
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < ldb; ++i) {
            const size_t e = (size_t)j * ldb + i;
            if (i >= m) CHECK(std::memcmp(&got[e], &hB[e], sizeof(T)) == 0);  // the ldb padding: untouched
            else {
                changed += std::memcmp(&got[e], &hB[e], sizeof(T)) != 0;
                for (int c = 0; c < Ty<T>::comps; ++c) CHECK(std::isfinite(part(got[e], c)));  // no NaN of A's unused parts came through
            }
        }
    CHECK(changed > (size_t)m * n - 8);   // in place: B now holds X
    hipFree(A), hipFree(B1), hipFree(B2), hipFree(work);
    return 0;
}

// m = n = ka = 8, side = left, uplo = lower, op = N, non-unit: m n ka = 512.  A has a diagonal of +-2 and strictly lower entries in {-1, 0, 1}; X is a matrix
// of small even integers and B = A X / 2 is formed exactly, so that A X' = 2 B has the exact solution X' = X ... with alpha = 2
template <typename T> int exact(hipblasHandle_t handle) {
    const int n = 8, ldb = n + 3;
    std::mt19937 gen(4);
    auto small = [&] { return (double)((int)(gen() % 3) - 1); };
    std::vector<T> hA((size_t)n * n), hX((size_t)n * n), hB((size_t)ldb * n, sentinel<T>());
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) hA[(size_t)j * n + i] = i == j ? make<T>(gen() % 2 ? 2.0 : -2.0, 0.0) : make<T>(small(), Ty<T>::comps == 2 ? small() : 0.0);
    for (auto& x : hX) x = make<T>(2 * small(), Ty<T>::comps == 2 ? 2 * small() : 0.0);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            double sr = 0, si = 0;  // (Atri X)(i, j) from the lower triangle of A
            for (int l = 0; l <= i; ++l) {
                const T &a = hA[(size_t)l * n + i], &x = hX[(size_t)j * n + l];
                sr += part(a, 0) * part(x, 0) - part(a, 1) * part(x, 1);
                si += part(a, 0) * part(x, 1) + part(a, 1) * part(x, 0);
            }
            hB[(size_t)j * ldb + i] = make<T>(sr / 2, si / 2);
        }
    T *A = dev(hA), *B = dev(hB);
    const T alpha = make<T>(2, 0);
    CHECK(trsm(handle, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, HIPBLAS_DIAG_NON_UNIT, n, n, &alpha, A, n, B, ldb) == HIPBLAS_STATUS_SUCCESS);
    const std::vector<T> got = host(B, hB.size());
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < ldb; ++i) {
            const size_t e = (size_t)j * ldb + i;
            if (i >= n) {
                CHECK(std::memcmp(&got[e], &hB[e], sizeof(T)) == 0);
                continue;
            }
            const T& x = hX[(size_t)j * n + i];
            if (part(got[e], 0) != part(x, 0) || (Ty<T>::comps == 2 && part(got[e], 1) != part(x, 1)))
                std::printf("type %d (%d, %d): got (%g, %g), exact (%g, %g)\n", Ty<T>::code, i, j, part(got[e], 0), part(got[e], 1), part(x, 0), part(x, 1));
            CHECK(part(got[e], 0) == part(x, 0));
            if (Ty<T>::comps == 2) CHECK(part(got[e], 1) == part(x, 1));
        }
    hipFree(A), hipFree(B);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("FAILED: run me as `test_hook_trsm emu | exact [sdcz]`\n");
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
        if (emulated<float>(handle, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, HIPBLAS_DIAG_NON_UNIT, false)) return 1;
        if (emulated<double>(handle, HIPBLAS_SIDE_RIGHT, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_T, HIPBLAS_DIAG_UNIT, false)) return 1;
        if (emulated<double>(handle, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_N, HIPBLAS_DIAG_NON_UNIT, true)) return 1;
        if (emulated<hipComplex>(handle, HIPBLAS_SIDE_RIGHT, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_C, HIPBLAS_DIAG_NON_UNIT, false)) return 1;
        if (emulated<hipDoubleComplex>(handle, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_C, HIPBLAS_DIAG_UNIT, false)) return 1;
        std::printf("hooked hipblas{S,D,C,Z}trsm (+ Dtrsm_64), in place on B == direct gemmul8_trsm (bitwise), ldb padding untouched\n");
    } else {
        const char* which = argc > 2 ? argv[2] : "sdcz";
        if (std::strchr(which, 's') && exact<float>(handle)) return 1;
        if (std::strchr(which, 'd') && exact<double>(handle)) return 1;
        if (std::strchr(which, 'c') && exact<hipComplex>(handle)) return 1;
        if (std::strchr(which, 'z') && exact<hipDoubleComplex>(handle)) return 1;
        std::printf("hipblas?trsm (%s): exact small-integer result\n", which);
    }
    CHECK(hipblasDestroy(handle) == HIPBLAS_STATUS_SUCCESS);
    std::printf("ALL OK\n");
    return 0;
}
