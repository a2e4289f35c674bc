// hipblas{C,Z}her2k under LD_PRELOAD=libgemmul8.so (no counterpart in the reference, which hooks GEMM only).  Links hipBLAS + the HIP runtime only;
// the direct emulation is reached through dlsym on the preloaded library.
//   emu   (GEMMUL8_NUM_MOD_Z / _C set by the caller): hipblasZher2k, hipblasZher2k_64, hipblasCher2k, hipblasCher2k_64 with host scalars and
//         hipblasZher2k / hipblasCher2k_64 in HIPBLAS_POINTER_MODE_DEVICE == gemmul8_her2k (host scalars) bit for bit over the WHOLE sentinel-filled
//         C buffer: the stored triangle equal, the other triangle untouched
//   native <k> (GEMMUL8_BACKEND=1, GEMMUL8_MIN_FLOPS, GEMMUL8_NONFINITE=ieee, or k = 2^17 + 8): the call reaches the native routine -- small-integer
//         data, so the exact answer is known
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipblas/hipblas.h>

#include <complex>
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

using her2k_fn = int (*)(void*, int, int, int, int, size_t, size_t, const void*, const void*, size_t, const void*, size_t, const void*, void*, size_t, unsigned,
                         int, void*, double*);
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

// R = float (hipblasCher2k) or double (hipblasZher2k); the matrices are std::complex<R>, layout-compatible with hipComplex / hipDoubleComplex
template <typename R> hipblasStatus_t call(hipblasHandle_t handle, bool ilp64, hipblasFillMode_t uplo, hipblasOperation_t trans, int n, int k, const std::complex<R>* alpha,
                                           const std::complex<R>* A, int lda, const std::complex<R>* B, int ldb, const R* beta, std::complex<R>* C, int ldc) {
    if constexpr (sizeof(R) == 8) {
        using Z = hipDoubleComplex;
        return ilp64 ? hipblasZher2k_64(handle, uplo, trans, (int64_t)n, (int64_t)k, (const Z*)alpha, (const Z*)A, (int64_t)lda, (const Z*)B, (int64_t)ldb, beta, (Z*)C, (int64_t)ldc)
                     : hipblasZher2k(handle, uplo, trans, n, k, (const Z*)alpha, (const Z*)A, lda, (const Z*)B, ldb, beta, (Z*)C, ldc);
    } else {
        using Z = hipComplex;
        return ilp64 ? hipblasCher2k_64(handle, uplo, trans, (int64_t)n, (int64_t)k, (const Z*)alpha, (const Z*)A, (int64_t)lda, (const Z*)B, (int64_t)ldb, beta, (Z*)C, (int64_t)ldc)
                     : hipblasCher2k(handle, uplo, trans, n, k, (const Z*)alpha, (const Z*)A, lda, (const Z*)B, ldb, beta, (Z*)C, ldc);
    }
}

template <typename R> int emulated(hipblasHandle_t handle, her2k_fn direct, ws_fn wsize, int dtype, unsigned N, hipblasFillMode_t uplo, hipblasOperation_t trans, bool ilp64,
                                   bool scalars_dev) {
    using T = std::complex<R>;
    const int n = 300, k = 200, ldc = n + 7;
    const int lda = (trans == HIPBLAS_OP_N ? n : k) + 3, ldb = (trans == HIPBLAS_OP_N ? n : k) + 1, cols = trans == HIPBLAS_OP_N ? k : n;
    std::mt19937 gen(3);
    std::uniform_real_distribution<double> U(-0.5, 0.5);
    T sent;
    std::memset(&sent, 0xA5, sizeof sent);
    std::vector<T> hA((size_t)lda * cols), hB((size_t)ldb * cols), hC((size_t)ldc * n, sent);
    for (auto& x : hA) x = T((R)U(gen), (R)U(gen));
    for (auto& x : hB) x = T((R)(8 * U(gen)), (R)(8 * U(gen)));
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i)
            if (uplo == HIPBLAS_FILL_MODE_LOWER ? i >= j : i <= j) hC[(size_t)j * ldc + i] = T((R)U(gen), (R)U(gen));
    T *A = dev(hA), *B = dev(hB), *C1 = dev(hC), *C2 = dev(hC);
    const T alpha((R)0.75, (R)-0.25);
    const R beta = (R)-0.5;
    void* work;
    hipMalloc(&work, wsize(1, 0, n, n, k, N, 0, 0, nullptr, nullptr));  // the equivalent GEMM's
    CHECK(direct(nullptr, dtype, 0, (int)uplo, (int)trans, n, k, &alpha, A, lda, B, ldb, &beta, C2, ldc, N, 0, work, nullptr) == 0);
    T* dalpha = dev(std::vector<T>{alpha});
    R* dbeta = dev(std::vector<R>{beta});
    if (scalars_dev) CHECK(hipblasSetPointerMode(handle, HIPBLAS_POINTER_MODE_DEVICE) == HIPBLAS_STATUS_SUCCESS);
    const hipblasStatus_t st = call<R>(handle, ilp64, uplo, trans, n, k, scalars_dev ? dalpha : &alpha, A, lda, B, ldb, scalars_dev ? dbeta : &beta, C1, ldc);
    if (scalars_dev) CHECK(hipblasSetPointerMode(handle, HIPBLAS_POINTER_MODE_HOST) == HIPBLAS_STATUS_SUCCESS);
    CHECK(st == HIPBLAS_STATUS_SUCCESS);
    const std::vector<T> got = host(C1, hC.size()), ref = host(C2, hC.size());
    CHECK(std::memcmp(got.data(), ref.data(), got.size() * sizeof(T)) == 0);  // hooked == direct, bit for bit
    size_t changed = 0;
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < ldc; ++i) {
            const bool in = i < n && (uplo == HIPBLAS_FILL_MODE_LOWER ? i >= j : i <= j);
            const size_t e = (size_t)j * ldc + i;
            if (!in) CHECK(std::memcmp(&got[e], &hC[e], sizeof(T)) == 0);  // the other triangle and the padding: untouched
            else changed += std::memcmp(&got[e], &hC[e], sizeof(T)) != 0;
            if (in && i == j) CHECK(got[e].imag() == 0 && !std::signbit(got[e].imag()));
        }
    CHECK(changed > (size_t)n * (n + 1) / 2 - 8);
    hipFree(A), hipFree(B), hipFree(C1), hipFree(C2), hipFree(work), hipFree(dalpha), hipFree(dbeta);
    return 0;
}

template <typename R> int native_exact(hipblasHandle_t handle, int k) {
    using T = std::complex<R>;
    using Zi = std::complex<long long>;
    const int n = 8, ldc = n + 3;
    std::mt19937 gen(4);
    T sent;
    std::memset(&sent, 0xA5, sizeof sent);
    std::vector<T> hA((size_t)n * k), hB((size_t)n * k), hC((size_t)ldc * n, sent);
    for (auto& x : hA) x = T((R)((int)(gen() % 3) - 1), (R)((int)(gen() % 3) - 1));  // -1, 0, 1: every sum is an exact small integer in float and double
    for (auto& x : hB) x = T((R)((int)(gen() % 3) - 1), (R)((int)(gen() % 3) - 1));
    for (int j = 0; j < n; ++j)
        for (int i = j; i < n; ++i) hC[(size_t)j * ldc + i] = T((R)(i - j), (R)(i == j ? 0 : i + j));
    T *A = dev(hA), *B = dev(hB), *C = dev(hC);
    const T alpha((R)2, (R)1);
    const R beta = (R)3;
    CHECK(call<R>(handle, false, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, n, k, &alpha, A, n, B, n, &beta, C, ldc) == HIPBLAS_STATUS_SUCCESS);
    const std::vector<T> got = host(C, hC.size());
    auto I = [](const T& z) { return Zi((long long)z.real(), (long long)z.imag()); };
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < ldc; ++i) {
            const size_t e = (size_t)j * ldc + i;
            if (i < n && i >= j) {
                Zi w = 0, wt = 0;  // W_ij = sum A_ik conj(B_jk), W_ji
                for (int kk = 0; kk < k; ++kk) {
                    w += I(hA[(size_t)kk * n + i]) * std::conj(I(hB[(size_t)kk * n + j]));
                    wt += I(hA[(size_t)kk * n + j]) * std::conj(I(hB[(size_t)kk * n + i]));
                }
                const Zi al(2, 1);
                const Zi want = al * w + std::conj(al * wt) + Zi(3, 0) * Zi(i - j, i == j ? 0 : i + j);
                CHECK(got[e] == T((R)want.real(), (R)(i == j ? 0 : want.imag())));
            } else {
                CHECK(std::memcmp(&got[e], &hC[e], sizeof(T)) == 0);
            }
        }
    hipFree(A), hipFree(B), hipFree(C);
    return 0;
}

int main(int argc, char** argv) {
    auto direct = (her2k_fn)dlsym(RTLD_DEFAULT, "gemmul8_her2k");
    auto wsize = (ws_fn)dlsym(RTLD_DEFAULT, "gemmul8_work_size");
    if (!direct || !wsize || argc < 2) {
        std::printf("FAILED: run me as `test_hook_her2k emu | native <k>` with LD_PRELOAD=libgemmul8.so\n");
        return 1;
    }
    hipSetDevice(0);
    hipblasHandle_t handle;
    hipblasCreate(&handle);
    if (!std::strcmp(argv[1], "emu")) {
        const unsigned Nz = (unsigned)std::atoi(std::getenv("GEMMUL8_NUM_MOD_Z")), Nc = (unsigned)std::atoi(std::getenv("GEMMUL8_NUM_MOD_C"));
        if (emulated<double>(handle, direct, wsize, 3, Nz, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, false, false)) return 1;
        if (emulated<double>(handle, direct, wsize, 3, Nz, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_C, true, false)) return 1;
        if (emulated<float>(handle, direct, wsize, 2, Nc, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_N, false, false)) return 1;
        if (emulated<float>(handle, direct, wsize, 2, Nc, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_C, true, false)) return 1;
        if (emulated<double>(handle, direct, wsize, 3, Nz, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_N, false, true)) return 1;
        if (emulated<float>(handle, direct, wsize, 2, Nc, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, true, true)) return 1;
        std::printf("hooked hipblasZher2k / Cher2k (+ _64), host and device scalars == direct gemmul8_her2k (bitwise), other triangle untouched\n");
    } else {
        const int k = argc > 2 ? std::atoi(argv[2]) : 64;
        if (native_exact<double>(handle, k)) return 1;
        if (native_exact<float>(handle, k)) return 1;
        std::printf("hipblasZher2k / Cher2k with k = %d passed to the native routine (exact small-integer result)\n", k);
    }
    CHECK(hipblasDestroy(handle) == HIPBLAS_STATUS_SUCCESS);
    std::printf("ALL OK\n");
    return 0;
}
