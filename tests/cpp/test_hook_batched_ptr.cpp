// The pointer-array batched GEMMs through the hook, with the program LINKED against libgemmul8.so in front of hipBLAS and rocBLAS (INTEGRATION.md
// "link-time": no LD_PRELOAD anywhere).  The caller sets GEMMUL8_NUM_MOD_* and reads the stats line (GEMMUL8_HOOK_STATS=1) to see which routine served.
//   emu      hipblasDgemmBatched, hipblasZgemmBatched, hipblasGemmBatchedEx (float32) and hipblasDgemmBatched_64 on 7 scattered items == direct
//            gemmul8_gemm per item, bit for bit over the whole sentinel-padded C buffers
//   chunks   the same three calls with GEMMUL8_BATCH_WORKSPACE_MB set (by the program, per type, from gemmul8_batched_item_bytes) so that exactly
//            three items fit the buffer: chunks of 3 + 3 + 1 items
//   exact    hipblasDgemmBatched twice on small-integer data whose product is exact whichever routine -- native or emulated -- serves the call
//   rocblas  rocblas_dgemm_batched (GEMMUL8_HOOK_ROCBLAS=1 by the caller) == direct gemmul8_gemm per item, bit for bit
#include <hip/hip_runtime.h>
#include <hipblas/hipblas.h>
#include <rocblas/rocblas.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/gemmul8_c.h"

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            return 1;                                                  \
        }                                                              \
    } while (0)

template <typename T> struct Ty;
template <> struct Ty<float> {
    static constexpr int code = GEMMUL8_S, comps = 1;
    static constexpr const char* env = "GEMMUL8_NUM_MOD_S";
};
template <> struct Ty<double> {
    static constexpr int code = GEMMUL8_D, comps = 1;
    static constexpr const char* env = "GEMMUL8_NUM_MOD_D";
};
template <> struct Ty<hipDoubleComplex> {
    static constexpr int code = GEMMUL8_Z, comps = 2;
    static constexpr const char* env = "GEMMUL8_NUM_MOD_Z";
};

enum Entry { kTyped, kTyped64, kEx, kRocblas };

inline hipblasStatus_t typed(hipblasHandle_t h, hipblasOperation_t ta, hipblasOperation_t tb, int m, int n, int k, const double* al, const double* const* A, int lda,
                             const double* const* B, int ldb, const double* be, double* const* C, int ldc, int batch, bool ilp64) {
    return ilp64 ? hipblasDgemmBatched_64(h, ta, tb, m, n, k, al, A, lda, B, ldb, be, C, ldc, batch) : hipblasDgemmBatched(h, ta, tb, m, n, k, al, A, lda, B, ldb, be, C, ldc, batch);
}
inline hipblasStatus_t typed(hipblasHandle_t h, hipblasOperation_t ta, hipblasOperation_t tb, int m, int n, int k, const hipDoubleComplex* al,
                             const hipDoubleComplex* const* A, int lda, const hipDoubleComplex* const* B, int ldb, const hipDoubleComplex* be,
                             hipDoubleComplex* const* C, int ldc, int batch, bool) {
    return hipblasZgemmBatched(h, ta, tb, m, n, k, al, A, lda, B, ldb, be, C, ldc, batch);
}
inline hipblasStatus_t typed(hipblasHandle_t, hipblasOperation_t, hipblasOperation_t, int, int, int, const float*, const float* const*, int, const float* const*, int,
                             const float*, float* const*, int, int, bool) {
    return HIPBLAS_STATUS_NOT_SUPPORTED;  // float32 goes through hipblasGemmBatchedEx here
}

// `batch` items, each operand in an allocation of its own (made in a scrambled order), odd items one element behind the allocation's start, ld = rows + 3;
// the hooked entry against gemmul8_gemm per item on twins of the C buffers
template <typename T> int scattered(hipblasHandle_t handle, Entry entry, hipblasOperation_t ta, hipblasOperation_t tb, int m, int n, int k, int batch) {
    using R = typename std::conditional<std::is_same<T, float>::value, float, double>::type;
    constexpr int CP = Ty<T>::comps;
    const unsigned N = (unsigned)std::atoi(std::getenv(Ty<T>::env));
    const int ra = ta == HIPBLAS_OP_N ? m : k, ca = ta == HIPBLAS_OP_N ? k : m, rb = tb == HIPBLAS_OP_N ? k : n, cb = tb == HIPBLAS_OP_N ? n : k;
    const int lda = ra + 3, ldb = rb + 3, ldc = m + 3;
    std::mt19937 gen(5);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    std::vector<const T*> pA(batch), pB(batch);
    std::vector<T*> pC(batch), pC2(batch);
    std::vector<void*> allocs;
    std::vector<std::vector<R>> hC(batch);
    const size_t nA = (size_t)lda * ca + 1, nB = (size_t)ldb * cb + 1, nC = (size_t)ldc * n + 1;
    for (int i = 0; i < batch; ++i) {
        const int b = (i * 3 + 2) % batch;  // allocation order: addresses do not ascend with the item index (batch = 7: a permutation)
        const size_t off = b & 1;
        std::vector<R> hA(nA * CP), hB(nB * CP);
        hC[b].resize(nC * CP);
        for (auto& x : hA) x = (R)(U(gen) * (1 + b));
        for (auto& x : hB) x = (R)U(gen);
        for (auto& x : hC[b]) x = (R)U(gen);
        T *dA, *dB, *dC, *dC2;
        CHECK(hipMalloc(&dA, nA * sizeof(T)) == hipSuccess && hipMalloc(&dB, nB * sizeof(T)) == hipSuccess && hipMalloc(&dC, nC * sizeof(T)) == hipSuccess &&
              hipMalloc(&dC2, nC * sizeof(T)) == hipSuccess);
        hipMemcpy(dA, hA.data(), nA * sizeof(T), hipMemcpyHostToDevice), hipMemcpy(dB, hB.data(), nB * sizeof(T), hipMemcpyHostToDevice);
        hipMemcpy(dC, hC[b].data(), nC * sizeof(T), hipMemcpyHostToDevice), hipMemcpy(dC2, hC[b].data(), nC * sizeof(T), hipMemcpyHostToDevice);
        pA[b] = dA + off, pB[b] = dB + off, pC[b] = dC + off, pC2[b] = dC2 + off;
        for (void* p : {(void*)dA, (void*)dB, (void*)dC, (void*)dC2}) allocs.push_back(p);
    }
    const T** dpA;
    const T** dpB;
    T** dpC;
    hipMalloc(&dpA, batch * sizeof(T*)), hipMalloc(&dpB, batch * sizeof(T*)), hipMalloc(&dpC, batch * sizeof(T*));
    hipMemcpy(dpA, pA.data(), batch * sizeof(T*), hipMemcpyHostToDevice), hipMemcpy(dpB, pB.data(), batch * sizeof(T*), hipMemcpyHostToDevice);
    hipMemcpy(dpC, pC.data(), batch * sizeof(T*), hipMemcpyHostToDevice);
    const R al[2] = {(R)-1.5, CP == 2 ? (R)0.5 : (R)0}, be[2] = {(R)0.5, CP == 2 ? (R)-0.25 : (R)0};
    void* work;
    hipMalloc(&work, gemmul8_work_size(CP == 2, GEMMUL8_INT8, m, n, k, N, 0, 0, nullptr, nullptr));
    for (int b = 0; b < batch; ++b)
        CHECK(gemmul8_gemm(nullptr, Ty<T>::code, GEMMUL8_INT8, (int)ta, (int)tb, m, n, k, al, pA[b], lda, pB[b], ldb, be, pC2[b], ldc, N, 0, work, nullptr, nullptr, 0,
                           0, 0, 0, nullptr) == 0);
    hipDeviceSynchronize();
    if (entry == kEx) {
        const hipDataType t = std::is_same<T, float>::value ? HIP_R_32F : std::is_same<T, double>::value ? HIP_R_64F : HIP_C_64F;
        const hipblasComputeType_t ct = std::is_same<T, float>::value ? HIPBLAS_COMPUTE_32F : HIPBLAS_COMPUTE_64F;
        CHECK(hipblasGemmBatchedEx(handle, ta, tb, m, n, k, al, (const void**)dpA, t, lda, (const void**)dpB, t, ldb, be, (void**)dpC, t, ldc, batch, ct,
                                   HIPBLAS_GEMM_DEFAULT) == HIPBLAS_STATUS_SUCCESS);
    } else if (entry == kRocblas) {
        if constexpr (std::is_same<T, double>::value) {
            rocblas_handle rh;
            CHECK(rocblas_create_handle(&rh) == rocblas_status_success);
            CHECK(rocblas_dgemm_batched(rh, (rocblas_operation)ta, (rocblas_operation)tb, m, n, k, al, dpA, lda, dpB, ldb, be, dpC, ldc, batch) == rocblas_status_success);
            hipDeviceSynchronize();
            CHECK(rocblas_destroy_handle(rh) == rocblas_status_success);
        } else {
            CHECK(false);
        }
    } else {
        CHECK(typed(handle, ta, tb, m, n, k, (const T*)al, dpA, lda, dpB, ldb, (const T*)be, dpC, ldc, batch, entry == kTyped64) == HIPBLAS_STATUS_SUCCESS);
    }
    hipDeviceSynchronize();
    size_t changed = 0;
    for (int b = 0; b < batch; ++b) {
        const size_t off = b & 1;
        std::vector<R> got(nC * CP), ref(nC * CP);
        hipMemcpy(got.data(), pC[b] - off, nC * sizeof(T), hipMemcpyDeviceToHost), hipMemcpy(ref.data(), pC2[b] - off, nC * sizeof(T), hipMemcpyDeviceToHost);
        CHECK(std::memcmp(got.data(), ref.data(), nC * sizeof(T)) == 0);  // hooked == direct, bit for bit, padding included
        for (size_t e = 0; e < nC; ++e) {
            const bool inside = e >= off && (e - off) % ldc < (size_t)m && (e - off) / ldc < (size_t)n;
            const bool same = std::memcmp(&got[e * CP], &hC[b][e * CP], sizeof(T)) == 0;
            if (!inside) CHECK(same);  // nothing outside the m x n window is written
            else changed += !same;
        }
    }
    CHECK(changed > (size_t)batch * m * n - 8);
    for (void* p : allocs) hipFree(p);
    hipFree(dpA), hipFree(dpB), hipFree(dpC), hipFree(work);
    return 0;
}

// item bytes >= 1 MiB: a whole number of MiB exists in [3 items, 4 items) -- exactly three items fit, 7 items run as chunks of 3 + 3 + 1
template <typename T> int three_chunks(hipblasHandle_t handle, Entry entry, int m, int n, int k) {
    const unsigned N = (unsigned)std::atoi(std::getenv(Ty<T>::env));
    const size_t item = gemmul8_batched_item_bytes(Ty<T>::comps == 2, GEMMUL8_INT8, m, n, k, N), mib = (size_t)1 << 20;
    CHECK(item >= mib);
    const size_t mb = (3 * item + mib - 1) / mib;
    CHECK(mb * mib / item == 3);
    setenv("GEMMUL8_BATCH_WORKSPACE_MB", std::to_string(mb).c_str(), 1);
    std::printf("type %d: item %zu bytes, GEMMUL8_BATCH_WORKSPACE_MB=%zu: 3 items per chunk\n", Ty<T>::code, item, mb);
    return scattered<T>(handle, entry, HIPBLAS_OP_N, HIPBLAS_OP_N, m, n, k, 7);
}

// 4 items of 8 x 8 x 8 with entries in {-1, 0, 1}: C = 2 A B + 3 C0 exactly, in any order of summation
int exact(hipblasHandle_t handle) {
    const int n = 8, batch = 4, ldc = n + 2;
    std::mt19937 gen(4);
    auto small = [&] { return (double)((int)(gen() % 3) - 1); };
    std::vector<double> hA((size_t)batch * n * n), hB((size_t)batch * n * n), hC((size_t)batch * ldc * n);
    for (auto& x : hA) x = small();
    for (auto& x : hB) x = small();
    for (auto& x : hC) x = small();
    double *dA, *dB, *dC;
    hipMalloc(&dA, hA.size() * 8), hipMalloc(&dB, hB.size() * 8), hipMalloc(&dC, hC.size() * 8);
    hipMemcpy(dA, hA.data(), hA.size() * 8, hipMemcpyHostToDevice), hipMemcpy(dB, hB.data(), hB.size() * 8, hipMemcpyHostToDevice);
    std::vector<const double*> pA(batch), pB(batch);
    std::vector<double*> pC(batch);
    for (int b = 0; b < batch; ++b) pA[b] = dA + (size_t)(batch - 1 - b) * n * n, pB[b] = dB + (size_t)b * n * n, pC[b] = dC + (size_t)b * ldc * n;
    const double** dpA;
    const double** dpB;
    double** dpC;
    hipMalloc(&dpA, batch * 8), hipMalloc(&dpB, batch * 8), hipMalloc(&dpC, batch * 8);
    hipMemcpy(dpA, pA.data(), batch * 8, hipMemcpyHostToDevice), hipMemcpy(dpB, pB.data(), batch * 8, hipMemcpyHostToDevice);
    hipMemcpy(dpC, pC.data(), batch * 8, hipMemcpyHostToDevice);
    const double al = 2.0, be = 3.0;
    for (int rep = 0; rep < 2; ++rep) {  // two calls: a message that is printed once is printed once
        hipMemcpy(dC, hC.data(), hC.size() * 8, hipMemcpyHostToDevice);
        CHECK(hipblasDgemmBatched(handle, HIPBLAS_OP_N, HIPBLAS_OP_N, n, n, n, &al, dpA, n, dpB, n, &be, dpC, ldc, batch) == HIPBLAS_STATUS_SUCCESS);
        hipDeviceSynchronize();
        std::vector<double> got(hC.size());
        hipMemcpy(got.data(), dC, hC.size() * 8, hipMemcpyDeviceToHost);
        for (int b = 0; b < batch; ++b)
            for (int j = 0; j < n; ++j)
                for (int i = 0; i < ldc; ++i) {
                    const size_t e = (size_t)b * ldc * n + (size_t)j * ldc + i;
                    double want = hC[e];
                    if (i < n) {
                        double s = 0;
                        for (int l = 0; l < n; ++l) s += hA[(size_t)(batch - 1 - b) * n * n + (size_t)l * n + i] * hB[(size_t)b * n * n + (size_t)j * n + l];
                        want = 2.0 * s + 3.0 * hC[e];
                    }
                    if (got[e] != want) std::printf("item %d (%d, %d): got %g, exact %g\n", b, i, j, got[e], want);
                    CHECK(got[e] == want);
                }
    }
    hipFree(dA), hipFree(dB), hipFree(dC), hipFree(dpA), hipFree(dpB), hipFree(dpC);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("FAILED: run me as `test_hook_batched_ptr emu | chunks | exact | rocblas`\n");
        return 1;
    }
    hipSetDevice(0);
    hipblasHandle_t handle;
    hipblasCreate(&handle);
    const std::string mode = argv[1];
    if (mode == "emu") {
        if (scattered<double>(handle, kTyped, HIPBLAS_OP_N, HIPBLAS_OP_N, 150, 70, 210, 7)) return 1;
        if (scattered<hipDoubleComplex>(handle, kTyped, HIPBLAS_OP_C, HIPBLAS_OP_T, 90, 70, 130, 7)) return 1;
        if (scattered<float>(handle, kEx, HIPBLAS_OP_T, HIPBLAS_OP_N, 150, 70, 210, 7)) return 1;
        if (scattered<double>(handle, kTyped64, HIPBLAS_OP_N, HIPBLAS_OP_T, 64, 33, 100, 7)) return 1;
        std::printf("hooked hipblasDgemmBatched(_64), hipblasZgemmBatched, hipblasGemmBatchedEx (float32) on 7 scattered items == direct gemmul8_gemm per item (bitwise)\n");
    } else if (mode == "chunks") {
        if (three_chunks<double>(handle, kTyped, 300, 200, 400)) return 1;
        if (three_chunks<hipDoubleComplex>(handle, kTyped, 300, 200, 400)) return 1;
        if (three_chunks<float>(handle, kEx, 300, 200, 700)) return 1;
        std::printf("three chunks == direct gemmul8_gemm per item (bitwise)\n");
    } else if (mode == "exact") {
        if (exact(handle)) return 1;
        std::printf("hipblasDgemmBatched: exact small-integer result\n");
    } else if (mode == "rocblas") {
        if (scattered<double>(handle, kRocblas, HIPBLAS_OP_N, HIPBLAS_OP_N, 150, 70, 210, 7)) return 1;
        std::printf("rocblas_dgemm_batched on 7 scattered items == direct gemmul8_gemm per item (bitwise)\n");
    } else {
        std::printf("FAILED: unknown mode %s\n", argv[1]);
        return 1;
    }
    CHECK(hipblasDestroy(handle) == HIPBLAS_STATUS_SUCCESS);
    std::printf("ALL OK\n");
    return 0;
}
