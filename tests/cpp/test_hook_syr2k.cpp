// hipblas{S,D}syr2k under LD_PRELOAD=libgemmul8.so (no counterpart in the reference, which hooks GEMM only).  Links hipBLAS + the HIP runtime only;
// the direct emulation is reached through dlsym on the preloaded library.
//   emu   (GEMMUL8_NUM_MOD_D / _S set by the caller): hipblasDsyr2k, hipblasDsyr2k_64 and hipblasSsyr2k(_64) == gemmul8_syr2k bit for bit over the
//         WHOLE sentinel-filled C buffer: the stored triangle equal, the other triangle untouched
//   native <k> (GEMMUL8_BACKEND=1, GEMMUL8_MIN_FLOPS, or k = 2^16 + 8): the call reaches the native routine -- small-integer data, so the exact
//         answer is known
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipblas/hipblas.h>

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

using syr2k_fn = int (*)(void*, int, int, int, int, size_t, size_t, const void*, const void*, size_t, const void*, size_t, const void*, void*, size_t, unsigned,
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
template <typename T> T sentinel() {
    T v;
    std::memset(&v, 0xA5, sizeof v);
    return v;
}

template <typename T> int emulated(hipblasHandle_t handle, syr2k_fn direct, ws_fn wsize, int dtype, unsigned N, hipblasFillMode_t uplo, hipblasOperation_t trans, bool ilp64) {
    const int n = 300, k = 200, ldc = n + 7;
    const int lda = (trans == HIPBLAS_OP_N ? n : k) + 3, ldb = (trans == HIPBLAS_OP_N ? n : k) + 1, cols = trans == HIPBLAS_OP_N ? k : n;
    std::mt19937 gen(3);
    std::uniform_real_distribution<double> U(-0.5, 0.5);
    std::vector<T> hA((size_t)lda * cols), hB((size_t)ldb * cols), hC((size_t)ldc * n, sentinel<T>());
    for (auto& x : hA) x = (T)U(gen);
    for (auto& x : hB) x = (T)(8 * U(gen));
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i)
            if (uplo == HIPBLAS_FILL_MODE_LOWER ? i >= j : i <= j) hC[(size_t)j * ldc + i] = (T)U(gen);
    T *A = dev(hA), *B = dev(hB), *C1 = dev(hC), *C2 = dev(hC);
    const T alpha = (T)0.75, beta = (T)-0.5;
    void* work;
    hipMalloc(&work, wsize(0, 0, n, n, 2 * ((k + 255) / 256 * 256), N, 0, 0, nullptr, nullptr));  // the equivalent GEMM's
    CHECK(direct(nullptr, dtype, 0, (int)uplo, (int)trans, n, k, &alpha, A, lda, B, ldb, &beta, C2, ldc, N, 0, work, nullptr) == 0);
    hipblasStatus_t st;
    if constexpr (sizeof(T) == 8) {
        st = ilp64 ? hipblasDsyr2k_64(handle, uplo, trans, (int64_t)n, (int64_t)k, &alpha, A, (int64_t)lda, B, (int64_t)ldb, &beta, C1, (int64_t)ldc)
                   : hipblasDsyr2k(handle, uplo, trans, n, k, &alpha, A, lda, B, ldb, &beta, C1, ldc);
    } else {
        st = ilp64 ? hipblasSsyr2k_64(handle, uplo, trans, (int64_t)n, (int64_t)k, &alpha, A, (int64_t)lda, B, (int64_t)ldb, &beta, C1, (int64_t)ldc)
                   : hipblasSsyr2k(handle, uplo, trans, n, k, &alpha, A, lda, B, ldb, &beta, C1, ldc);
    }
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
        }
    CHECK(changed > (size_t)n * (n + 1) / 2 - 8);
    hipFree(A), hipFree(B), hipFree(C1), hipFree(C2), hipFree(work);
    return 0;
}

template <typename T> int native_exact(hipblasHandle_t handle, int k) {
    const int n = 8, ldc = n + 3;
    std::mt19937 gen(4);
    std::vector<T> hA((size_t)n * k), hB((size_t)n * k), hC((size_t)ldc * n, sentinel<T>());
    for (auto& x : hA) x = (T)((int)(gen() % 3) - 1);  // -1, 0, 1: every sum is an exact small integer in float and double
    for (auto& x : hB) x = (T)((int)(gen() % 3) - 1);
    for (int j = 0; j < n; ++j)
        for (int i = j; i < n; ++i) hC[(size_t)j * ldc + i] = (T)(i - j);
    T *A = dev(hA), *B = dev(hB), *C = dev(hC);
    const T alpha = (T)2, beta = (T)3;
    hipblasStatus_t st;
    if constexpr (sizeof(T) == 8) st = hipblasDsyr2k(handle, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, n, k, &alpha, A, n, B, n, &beta, C, ldc);
    else st = hipblasSsyr2k(handle, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, n, k, &alpha, A, n, B, n, &beta, C, ldc);
    CHECK(st == HIPBLAS_STATUS_SUCCESS);
    const std::vector<T> got = host(C, hC.size());
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < ldc; ++i) {
            const size_t e = (size_t)j * ldc + i;
            if (i < n && i >= j) {
                long long s = 0;
                for (int kk = 0; kk < k; ++kk)
                    s += (long long)hA[(size_t)kk * n + i] * (long long)hB[(size_t)kk * n + j] + (long long)hB[(size_t)kk * n + i] * (long long)hA[(size_t)kk * n + j];
                CHECK(got[e] == (T)(2 * s + 3 * (i - j)));
            } else {
                CHECK(std::memcmp(&got[e], &hC[e], sizeof(T)) == 0);
            }
        }
    hipFree(A), hipFree(B), hipFree(C);
    return 0;
}

int main(int argc, char** argv) {
    auto direct = (syr2k_fn)dlsym(RTLD_DEFAULT, "gemmul8_syr2k");
    auto wsize = (ws_fn)dlsym(RTLD_DEFAULT, "gemmul8_work_size");
    if (!direct || !wsize || argc < 2) {
        std::printf("FAILED: run me as `test_hook_syr2k emu | native <k>` with LD_PRELOAD=libgemmul8.so\n");
        return 1;
    }
    hipSetDevice(0);
    hipblasHandle_t handle;
    hipblasCreate(&handle);
    if (!std::strcmp(argv[1], "emu")) {
        const unsigned Nd = (unsigned)std::atoi(std::getenv("GEMMUL8_NUM_MOD_D")), Ns = (unsigned)std::atoi(std::getenv("GEMMUL8_NUM_MOD_S"));
        if (emulated<double>(handle, direct, wsize, 1, Nd, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_N, false)) return 1;
        if (emulated<double>(handle, direct, wsize, 1, Nd, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_T, true)) return 1;
        if (emulated<float>(handle, direct, wsize, 0, Ns, HIPBLAS_FILL_MODE_UPPER, HIPBLAS_OP_N, false)) return 1;
        if (emulated<float>(handle, direct, wsize, 0, Ns, HIPBLAS_FILL_MODE_LOWER, HIPBLAS_OP_T, true)) return 1;
        std::printf("hooked hipblasDsyr2k / Ssyr2k (+ _64) == direct gemmul8_syr2k (bitwise), other triangle untouched\n");
    } else {
        const int k = argc > 2 ? std::atoi(argv[2]) : 64;
        if (native_exact<double>(handle, k)) return 1;
        if (native_exact<float>(handle, k)) return 1;
        std::printf("hipblasDsyr2k / Ssyr2k with k = %d passed to the native routine (exact small-integer result)\n", k);
    }
    CHECK(hipblasDestroy(handle) == HIPBLAS_STATUS_SUCCESS);
    std::printf("ALL OK\n");
    return 0;
}
