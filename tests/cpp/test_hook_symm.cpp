// hipblasDsymm / hipblasZhemm through the hook, with the program LINKED against libgemmul8.so in front of hipBLAS (INTEGRATION.md "link-time": no
// LD_PRELOAD anywhere): the hook's definitions of the hipBLAS names come first in the search order, the direct emulation is called by name.
//   emu          (GEMMUL8_NUM_MOD_D / _Z set by the caller): hipblasDsymm, hipblasDsymm_64, hipblasZhemm, hipblasZhemm_64 == gemmul8_symm / gemmul8_hemm bit
//                for bit over the WHOLE sentinel-filled C buffer; the unused triangle of A (and HEMM's diagonal imaginary parts) holds NaN
//   exact d|z|dz small-integer data, so the exact answer is known whichever routine -- native or emulated -- serves the call; the caller reads from the
//                stats lines which one did
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
inline double make(double re, double, double*) { return re; }
inline hipDoubleComplex make(double re, double im, hipDoubleComplex*) { return hipDoubleComplex(re, im); }
inline bool stored(hipblasFillMode_t uplo, int i, int j) { return uplo == HIPBLAS_FILL_MODE_LOWER ? i >= j : i <= j; }

// T = double: SYMM, T = hipDoubleComplex: HEMM
template <typename T> int emulated(hipblasHandle_t handle, unsigned N, hipblasSideMode_t side, hipblasFillMode_t uplo, bool ilp64) {
    constexpr bool herm = sizeof(T) == 16;
    const int m = 300, n = 200, ka = side == HIPBLAS_SIDE_LEFT ? m : n, lda = ka + 3, ldb = m + 1, ldc = m + 7;
    std::mt19937 gen(3);
    std::uniform_real_distribution<double> U(-0.5, 0.5);
    const double nan = std::nan("");
    std::vector<T> hA((size_t)lda * ka, make(nan, nan, (T*)nullptr)), hB((size_t)ldb * n), hC((size_t)ldc * n, sentinel<T>());
    for (int j = 0; j < ka; ++j)
        for (int i = 0; i < ka; ++i)
            if (stored(uplo, i, j)) hA[(size_t)j * lda + i] = make(U(gen), i == j ? nan : U(gen), (T*)nullptr);  // (HEMM ignores the diagonal's imaginary part)
    for (auto& x : hB) x = make(8 * U(gen), 8 * U(gen), (T*)nullptr);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < m; ++i) hC[(size_t)j * ldc + i] = make(U(gen), U(gen), (T*)nullptr);
    T *A = dev(hA), *B = dev(hB), *C1 = dev(hC), *C2 = dev(hC);
    const T alpha = make(0.75, -0.25, (T*)nullptr), beta = make(-0.5, 1.5, (T*)nullptr);
    void* work;
    hipMalloc(&work, gemmul8_work_size(herm, GEMMUL8_INT8, m, n, ka, N, 0, 0, nullptr, nullptr));  // the equivalent GEMM's
    hipblasStatus_t st;
    if constexpr (herm) {
        CHECK(gemmul8_hemm(nullptr, GEMMUL8_Z, GEMMUL8_INT8, (int)side, (int)uplo, m, n, &alpha, A, lda, B, ldb, &beta, C2, ldc, N, 0, work, nullptr) == 0);
        st = ilp64 ? hipblasZhemm_64(handle, side, uplo, (int64_t)m, (int64_t)n, &alpha, A, (int64_t)lda, B, (int64_t)ldb, &beta, C1, (int64_t)ldc)
                   : hipblasZhemm(handle, side, uplo, m, n, &alpha, A, lda, B, ldb, &beta, C1, ldc);
    } else {
        CHECK(gemmul8_symm(nullptr, GEMMUL8_D, GEMMUL8_INT8, (int)side, (int)uplo, m, n, &alpha, A, lda, B, ldb, &beta, C2, ldc, N, 0, work, nullptr) == 0);
        st = ilp64 ? hipblasDsymm_64(handle, side, uplo, (int64_t)m, (int64_t)n, &alpha, A, (int64_t)lda, B, (int64_t)ldb, &beta, C1, (int64_t)ldc)
                   : hipblasDsymm(handle, side, uplo, m, n, &alpha, A, lda, B, ldb, &beta, C1, ldc);
    }
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
                double parts[sizeof(T) / 8];
                std::memcpy(parts, &got[e], sizeof(T));
                for (double p : parts) CHECK(std::isfinite(p));  // no NaN of A's unused parts came through
            }
        }
    CHECK(changed > (size_t)m * n - 8);
    hipFree(A), hipFree(B), hipFree(C1), hipFree(C2), hipFree(work);
    return 0;
}

// m = n = ka = 8, side = left, uplo = lower: 2 m n ka = 1024
template <typename T> int exact(hipblasHandle_t handle) {
    constexpr bool herm = sizeof(T) == 16;
    const int n = 8, ldc = n + 3;
    std::mt19937 gen(4);
    auto small = [&] { return (double)((int)(gen() % 3) - 1); };  // -1, 0, 1: every sum is an exact small integer
    std::vector<T> hA((size_t)n * n), hB((size_t)n * n), hC((size_t)ldc * n, sentinel<T>());
    for (auto& x : hA) x = make(small(), small(), (T*)nullptr);
    for (auto& x : hB) x = make(small(), small(), (T*)nullptr);
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) hC[(size_t)j * ldc + i] = make(i - j, herm ? i + j : 0, (T*)nullptr);
    T *A = dev(hA), *B = dev(hB), *C = dev(hC);
    const T alpha = make(2, 0, (T*)nullptr), beta = make(3, 0, (T*)nullptr);
    hipblasStatus_t st;
    if constexpr (herm) st = hipblasZhemm(handle, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_LOWER, n, n, &alpha, A, n, B, n, &beta, C, ldc);
    else st = hipblasDsymm(handle, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_LOWER, n, n, &alpha, A, n, B, n, &beta, C, ldc);
    CHECK(st == HIPBLAS_STATUS_SUCCESS);
    const std::vector<T> got = host(C, hC.size());
    auto re = [](const T& v) { double p[sizeof(T) / 8]; std::memcpy(p, &v, sizeof(T)); return p[0]; };
    auto im = [](const T& v) { double p[2] = {0, 0}; std::memcpy(p, &v, sizeof(T)); return sizeof(T) == 16 ? p[1] : 0.0; };
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < ldc; ++i) {
            const size_t e = (size_t)j * ldc + i;
            if (i >= n) {
                CHECK(std::memcmp(&got[e], &hC[e], sizeof(T)) == 0);
                continue;
            }
            double sr = 0, si = 0;  // (Afull B)(i, j) from the lower triangle of A
            for (int l = 0; l < n; ++l) {
                const T& a = i >= l ? hA[(size_t)l * n + i] : hA[(size_t)i * n + l];
                const double ar = re(a), ai = !herm || i == l ? 0.0 : (i >= l ? im(a) : -im(a));
                const double air = herm ? ai : im(a);
                const T& b = hB[(size_t)j * n + l];
                sr += ar * re(b) - air * im(b);
                si += ar * im(b) + air * re(b);
            }
            CHECK(re(got[e]) == 2 * sr + 3 * re(hC[e]));
            CHECK(im(got[e]) == 2 * si + 3 * im(hC[e]));
        }
    hipFree(A), hipFree(B), hipFree(C);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("FAILED: run me as `test_hook_symm emu | exact d|z|dz`\n");
        return 1;
    }
    hipSetDevice(0);
    hipblasHandle_t handle;
    hipblasCreate(&handle);
    if (!std::strcmp(argv[1], "emu")) {
        const unsigned Nd = (unsigned)std::atoi(std::getenv("GEMMUL8_NUM_MOD_D")), Nz = (unsigned)std::atoi(std::getenv("GEMMUL8_NUM_MOD_Z"));
        if (emulated<double>(handle, Nd, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_LOWER, false)) return 1;
        if (emulated<double>(handle, Nd, HIPBLAS_SIDE_RIGHT, HIPBLAS_FILL_MODE_UPPER, true)) return 1;
        if (emulated<hipDoubleComplex>(handle, Nz, HIPBLAS_SIDE_LEFT, HIPBLAS_FILL_MODE_UPPER, false)) return 1;
        if (emulated<hipDoubleComplex>(handle, Nz, HIPBLAS_SIDE_RIGHT, HIPBLAS_FILL_MODE_LOWER, true)) return 1;
        std::printf("hooked hipblasDsymm / Zhemm (+ _64) == direct gemmul8_symm / gemmul8_hemm (bitwise), ldc padding untouched\n");
    } else {
        const char* which = argc > 2 ? argv[2] : "dz";
        if (std::strchr(which, 'd') && exact<double>(handle)) return 1;
        if (std::strchr(which, 'z') && exact<hipDoubleComplex>(handle)) return 1;
        std::printf("hipblasDsymm / Zhemm (%s): exact small-integer result\n", which);
    }
    CHECK(hipblasDestroy(handle) == HIPBLAS_STATUS_SUCCESS);
    std::printf("ALL OK\n");
    return 0;
}
