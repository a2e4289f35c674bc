// hipblas{C,Z}herk under LD_PRELOAD=libgemmul8.so (no counterpart in the reference, which hooks GEMM only).  Links hipBLAS + the HIP runtime only;
// the direct emulation is reached through dlsym on the preloaded library.
//   emu   (GEMMUL8_NUM_MOD_Z / _C set by the caller): hipblasZherk, hipblasZherk_64 and hipblasCherk == gemmul8_herk bit for bit over the WHOLE
//         sentinel-filled C buffer: the stored triangle equal, the other triangle untouched, the diagonal's imaginary parts +0.0 although they came in as NaN
//   native <k> (GEMMUL8_BACKEND=1, or k = 2^17 + 8): the call reaches the native routine -- small-integer data, so the exact answer is known
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipblas/hipblas.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                  \
        }                                                              \
    } while (0)

using herk_fn = int (*)(void*, int, int, int, int, size_t, size_t, const void*, const void*, size_t, const void*, void*, size_t, unsigned, int, void*,
                        double*);
using ws_fn = size_t (*)(int, int, size_t, size_t, size_t, unsigned, int, int, size_t*, size_t*);

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

// R = float / double; a complex element is two R (the layout of hipComplex / hipDoubleComplex)
template <typename R> struct Cx {
    R re, im;
};
template <typename R> Cx<R> sentinel() {
    Cx<R> v;
    std::memset(&v, 0xA5, sizeof v);
    return v;
}

template <typename R> hipblasStatus_t herk(hipblasHandle_t h, hipblasFillMode_t uplo, hipblasOperation_t trans, int n, int k, const R* alpha, const Cx<R>* A, int lda,
                                           const R* beta, Cx<R>* C, int ldc, bool ilp64) {
    if constexpr (sizeof(R) == 8) {
        auto *a = (const hipDoubleComplex*)A;
        auto *c = (hipDoubleComplex*)C;
        return ilp64 ? hipblasZherk_64(h, uplo, trans, (int64_t)n, (int64_t)k, alpha, a, (int64_t)lda, beta, c, (int64_t)ldc)
                     : hipblasZherk(h, uplo, trans, n, k, alpha, a, lda, beta, c, ldc);
    } else {
        auto *a = (const hipComplex*)A;
        auto *c = (hipComplex*)C;
        return ilp64 ? hipblasCherk_64(h, uplo, trans, (int64_t)n, (int64_t)k, alpha, a, (int64_t)lda, beta, c, (int64_t)ldc)
                     : hipblasCherk(h, uplo, trans, n, k, alpha, a, lda, beta, c, ldc);
    }
}

template <typename R> int emulated(hipblasHandle_t handle, herk_fn direct, ws_fn wsize, int dtype, unsigned N, hipblasFillMode_t uplo, hipblasOperation_t trans, bool ilp64) {
    using T = Cx<R>;
    const int n = 300, k = 200, ldc = n + 7;
    const int lda = trans == HIPBLAS_OP_N ? n : k;
    std::mt19937 gen(3);
    std::uniform_real_distribution<double> U(-0.5, 0.5);
    std::vector<T> hA((size_t)n * k), hC((size_t)ldc * n, sentinel<R>());
    for (auto& x : hA) x = T{(R)U(gen), (R)U(gen)};
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i)
            if (uplo == HIPBLAS_FILL_MODE_LOWER ? i >= j : i <= j) hC[(size_t)j * ldc + i] = T{(R)U(gen), i == j ? (R)NAN : (R)U(gen)};
    T *A = dev(hA), *C1 = dev(hC), *C2 = dev(hC);
    const R alpha = (R)0.75, beta = (R)-0.5;
    void* work;
    hipMalloc(&work, wsize(1, 0, n, n, k, N, 0, 0, nullptr, nullptr));
    CHECK(direct(nullptr, dtype, 0, (int)uplo, (int)trans, n, k, &alpha, A, lda, &beta, C2, ldc, N, 0, work, nullptr) == 0);
    CHECK(herk<R>(handle, uplo, trans, n, k, &alpha, A, lda, &beta, C1, ldc, ilp64) == HIPBLAS_STATUS_SUCCESS);
    const std::vector<T> got = host(C1, hC.size()), ref = host(C2, hC.size());
    CHECK(std::memcmp(got.data(), ref.data(), got.size() * sizeof(T)) == 0);  // hooked == direct, bit for bit
    size_t changed = 0;
    const R zero = 0;
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < ldc; ++i) {
            const bool in = i < n && (uplo == HIPBLAS_FILL_MODE_LOWER ? i >= j : i <= j);
            const size_t e = (size_t)j * ldc + i;
            if (!in) CHECK(std::memcmp(&got[e], &hC[e], sizeof(T)) == 0);  // the other triangle and the padding: untouched
            else changed += std::memcmp(&got[e], &hC[e], sizeof(T)) != 0;
            if (in && i == j) CHECK(std::memcmp(&got[e].im, &zero, sizeof(R)) == 0 && std::isfinite((double)got[e].re));  // +0.0; the NaN reached neither part
        }
    CHECK(changed > (size_t)n * (n + 1) / 2 - 8);
    hipFree(A), hipFree(C1), hipFree(C2), hipFree(work);
    return 0;
}

template <typename R> int native_exact(hipblasHandle_t handle, int k) {
    using T = Cx<R>;
    const int n = 8, ldc = n + 3;
    std::mt19937 gen(4);
    std::vector<T> hA((size_t)n * k), hC((size_t)ldc * n, sentinel<R>());
    for (auto& x : hA) x = T{(R)((int)(gen() % 3) - 1), (R)((int)(gen() % 3) - 1)};  // -1, 0, 1: every sum is an exact small integer in float and double
    for (int j = 0; j < n; ++j)
        for (int i = j; i < n; ++i) hC[(size_t)j * ldc + i] = T{(R)(i - j), (R)(i == j ? 0 : i + j)};
    T *A = dev(hA), *C = dev(hC);
    const R alpha = (R)2, beta = (R)3;
    CHECK(herk<R>(handle, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, n, k, &alpha, A, n, &beta, C, ldc, false) == HIPBLAS_STATUS_SUCCESS);
    const std::vector<T> got = host(C, hC.size());
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < ldc; ++i) {
            const size_t e = (size_t)j * ldc + i;
            if (i < n && i >= j) {
                long long sr = 0, si = 0;  // sum over kk of a[i] * conj(a[j])
                for (int kk = 0; kk < k; ++kk) {
                    const T x = hA[(size_t)kk * n + i], y = hA[(size_t)kk * n + j];
                    sr += (long long)x.re * (long long)y.re + (long long)x.im * (long long)y.im;
                    si += (long long)x.im * (long long)y.re - (long long)x.re * (long long)y.im;
                }
                CHECK(got[e].re == (R)(2 * sr + 3 * (i - j)));
                CHECK(got[e].im == (R)(i == j ? 0 : 2 * si + 3 * (i + j)));
            } else {
                CHECK(std::memcmp(&got[e], &hC[e], sizeof(T)) == 0);
            }
        }
    hipFree(A), hipFree(C);
    return 0;
}

int main(int argc, char** argv) {
    auto direct = (herk_fn)dlsym(RTLD_DEFAULT, "gemmul8_herk");
    auto wsize = (ws_fn)dlsym(RTLD_DEFAULT, "gemmul8_work_size");
    if (!direct || !wsize || argc < 2) {
        std::printf("FAILED: run me as `test_hook_herk emu | native <k>` with LD_PRELOAD=libgemmul8.so\n");
        return 1;
    }
    hipSetDevice(0);
    hipblasHandle_t handle;
    hipblasCreate(&handle);
    if (!std::strcmp(argv[1], "emu")) {
        const unsigned Nz = (unsigned)std::atoi(std::getenv("GEMMUL8_NUM_MOD_Z")), Nc = (unsigned)std::atoi(std::getenv("GEMMUL8_NUM_MOD_C"));
        if (emulated<double>(handle, direct, wsize, 3, Nz, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, false)) return 1;
        if (emulated<double>(handle, direct, wsize, 3, Nz, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_C, true)) return 1;
        if (emulated<float>(handle, direct, wsize, 2, Nc, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_N, false)) return 1;
        if (emulated<float>(handle, direct, wsize, 2, Nc, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_C, false)) return 1;
        std::printf("hooked hipblasZherk / Cherk (+ _64) == direct gemmul8_herk (bitwise), other triangle untouched\n");
    } else {
        const int k = argc > 2 ? std::atoi(argv[2]) : 64;
        if (native_exact<double>(handle, k)) return 1;
        if (native_exact<float>(handle, k)) return 1;
        std::printf("hipblasZherk / Cherk with k = %d passed to the native routine (exact small-integer result)\n", k);
    }
    CHECK(hipblasDestroy(handle) == HIPBLAS_STATUS_SUCCESS);
    std::printf("ALL OK\n");
    return 0;
}
