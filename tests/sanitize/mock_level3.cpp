// TEST INFRASTRUCTURE for tests/test_hook_level3_gate.py, linked in addition to mock_gpu.cpp: what that mock lacks on purpose -- the Level-3 entries of
// the libgemmul8 C ABI (gemmul8_syrk / herk / syr2k / her2k / symm / hemm / trmm / trsm, gemmul8_trsm_work_size, gemmul8_set_nonfinite_mode) and the
// "real" hipBLAS routines behind the 52 Level-3 names oz2_hook.cpp interposes.  Every entry prints one line to stdout with its name and every scalar
// argument; a matrix pointer prints as the name of a buffer the driver registered plus a byte offset, the workspace as null / non-null: no address
// appears, so the output of a run is the same text every time and level3_driver.cpp's transcript can be compared byte for byte.
// Each ABI entry writes the LAST byte of the workspace it is entitled to (the mock's gemmul8_work_size for the equivalent GEMM, its own
// gemmul8_trsm_work_size for TRSM): a workspace the hook grew too short is a sanitizer error.  MOCK_LEVEL3_RC is the status the ABI entries return.
// -DMOCK_LEVEL3_NATIVES_ONLY: the natives alone, for "the library lacks the entry point".
// Built with the sanitizer flags of the hook and the driver.  No matrix is ever dereferenced: the driver passes dimensions far larger than its buffers.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipblas/hipblas.h>
#include <sys/mman.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gemmul8_c.h"

#define EXPORT extern "C" __attribute__((visibility("default")))

namespace {
struct Region { std::string name; const char* base; size_t bytes; };
std::vector<Region> g_regions;

std::string P(const void* p) {
    if (!p) return "null";
    for (const Region& r : g_regions)
        if ((const char*)p >= r.base && (const char*)p < r.base + r.bytes) return r.name + "+" + std::to_string((const char*)p - r.base);
    return "unregistered";
}
std::string V(const float* s) { return s ? std::to_string(*s) : "null"; }
std::string V(const double* s) { return s ? std::to_string(*s) : "null"; }
std::string V(const hipComplex* s) { return s ? "(" + std::to_string(s->x) + "," + std::to_string(s->y) + ")" : "null"; }
std::string V(const hipDoubleComplex* s) { return s ? "(" + std::to_string(s->x) + "," + std::to_string(s->y) + ")" : "null"; }
#define S(x) (x).c_str()
typedef long long ll;
}  // namespace

EXPORT void mock_level3_register(const char* name, const void* base, size_t bytes) { g_regions.push_back({name, (const char*)base, bytes}); }

// ---- workspaces of 64 MiB and more (the order-2^17 cases ask for tens of GiB) bypass malloc, whose sanitizer shadow would cost an eighth of the
// size in touched memory: an untouched private mapping that ENDS at an inaccessible MiB, so a write past the end still faults.  Smaller ones go on
// to mock_gpu.cpp's malloc.
namespace {
std::mutex g_big_mtx;
std::map<void*, std::pair<void*, size_t>> g_big;  // user pointer -> mapping
constexpr size_t kBig = size_t(64) << 20;
bool free_big(void* p) {
    std::lock_guard<std::mutex> g(g_big_mtx);
    auto it = g_big.find(p);
    if (it == g_big.end()) return false;
    munmap(it->second.first, it->second.second);
    g_big.erase(it);
    return true;
}
using MallocAsync = hipError_t (*)(void**, size_t, hipStream_t);
using FreeAsync = hipError_t (*)(void*, hipStream_t);
using Free = hipError_t (*)(void*);
template <typename Fn> Fn next(const char* name) { return reinterpret_cast<Fn>(dlsym(RTLD_NEXT, name)); }
}  // namespace
EXPORT hipError_t hipMallocAsync(void** p, size_t n, hipStream_t s) {
    if (n < kBig) return next<MallocAsync>("hipMallocAsync")(p, n, s);
    const size_t page = (size_t)sysconf(_SC_PAGESIZE), guard = size_t(1) << 20, len = (n + page - 1) / page * page + guard;
    void* map = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (map == MAP_FAILED) return hipErrorOutOfMemory;
    mprotect((char*)map + len - guard, guard, PROT_NONE);
    *p = (char*)map + len - guard - n;
    std::lock_guard<std::mutex> g(g_big_mtx);
    g_big[*p] = {map, len};
    return hipSuccess;
}
EXPORT hipError_t hipFreeAsync(void* p, hipStream_t s) { return free_big(p) ? hipSuccess : next<FreeAsync>("hipFreeAsync")(p, s); }
EXPORT hipError_t hipFree(void* p) { return free_big(p) ? hipSuccess : next<Free>("hipFree")(p); }

// ---- the "real" hipBLAS Level-3 routines: print and succeed
#define NATIVE_RANK1(NAME, T, R, I)                                                                                                             \
    EXPORT hipblasStatus_t NAME(hipblasHandle_t, hipblasFillMode_t uplo, hipblasOperation_t trans, I n, I k, const R* alpha, const T* A, I lda,  \
                                const R* beta, T* C, I ldc) {                                                                                   \
        std::printf("native " #NAME " uplo=%d trans=%d n=%lld k=%lld alpha=%s A=%s lda=%lld beta=%s C=%s ldc=%lld\n", (int)uplo, (int)trans, (ll)n, \
                    (ll)k, S(V(alpha)), S(P(A)), (ll)lda, S(V(beta)), S(P(C)), (ll)ldc);                                                        \
        return HIPBLAS_STATUS_SUCCESS;                                                                                                          \
    }
#define NATIVE_RANK2(NAME, T, R, I)                                                                                                             \
    EXPORT hipblasStatus_t NAME(hipblasHandle_t, hipblasFillMode_t uplo, hipblasOperation_t trans, I n, I k, const T* alpha, const T* A, I lda,  \
                                const T* B, I ldb, const R* beta, T* C, I ldc) {                                                                \
        std::printf("native " #NAME " uplo=%d trans=%d n=%lld k=%lld alpha=%s A=%s lda=%lld B=%s ldb=%lld beta=%s C=%s ldc=%lld\n", (int)uplo,   \
                    (int)trans, (ll)n, (ll)k, S(V(alpha)), S(P(A)), (ll)lda, S(P(B)), (ll)ldb, S(V(beta)), S(P(C)), (ll)ldc);                   \
        return HIPBLAS_STATUS_SUCCESS;                                                                                                          \
    }
#define NATIVE_SYMM(NAME, T, I)                                                                                                                 \
    EXPORT hipblasStatus_t NAME(hipblasHandle_t, hipblasSideMode_t side, hipblasFillMode_t uplo, I m, I n, const T* alpha, const T* A, I lda,    \
                                const T* B, I ldb, const T* beta, T* C, I ldc) {                                                                \
        std::printf("native " #NAME " side=%d uplo=%d m=%lld n=%lld alpha=%s A=%s lda=%lld B=%s ldb=%lld beta=%s C=%s ldc=%lld\n", (int)side,    \
                    (int)uplo, (ll)m, (ll)n, S(V(alpha)), S(P(A)), (ll)lda, S(P(B)), (ll)ldb, S(V(beta)), S(P(C)), (ll)ldc);                    \
        return HIPBLAS_STATUS_SUCCESS;                                                                                                          \
    }
#define NATIVE_TRMM(NAME, T, I)                                                                                                                 \
    EXPORT hipblasStatus_t NAME(hipblasHandle_t, hipblasSideMode_t side, hipblasFillMode_t uplo, hipblasOperation_t trans, hipblasDiagType_t diag, \
                                I m, I n, const T* alpha, const T* A, I lda, const T* B, I ldb, T* C, I ldc) {                                  \
        std::printf("native " #NAME " side=%d uplo=%d trans=%d diag=%d m=%lld n=%lld alpha=%s A=%s lda=%lld B=%s ldb=%lld C=%s ldc=%lld\n",     \
                    (int)side, (int)uplo, (int)trans, (int)diag, (ll)m, (ll)n, S(V(alpha)), S(P(A)), (ll)lda, S(P(B)), (ll)ldb, S(P(C)), (ll)ldc); \
        return HIPBLAS_STATUS_SUCCESS;                                                                                                          \
    }
#define NATIVE_TRSM(NAME, T, I)                                                                                                                 \
    EXPORT hipblasStatus_t NAME(hipblasHandle_t, hipblasSideMode_t side, hipblasFillMode_t uplo, hipblasOperation_t trans, hipblasDiagType_t diag, \
                                I m, I n, const T* alpha, const T* A, I lda, T* B, I ldb) {                                                     \
        std::printf("native " #NAME " side=%d uplo=%d trans=%d diag=%d m=%lld n=%lld alpha=%s A=%s lda=%lld B=%s ldb=%lld\n", (int)side,         \
                    (int)uplo, (int)trans, (int)diag, (ll)m, (ll)n, S(V(alpha)), S(P(A)), (ll)lda, S(P(B)), (ll)ldb);                           \
        return HIPBLAS_STATUS_SUCCESS;                                                                                                          \
    }
#define NATIVE_TYPE(U, T)                                                                      \
    NATIVE_RANK1(hipblas##U##syrk, T, T, int) NATIVE_RANK1(hipblas##U##syrk_64, T, T, int64_t)   \
    NATIVE_RANK2(hipblas##U##syr2k, T, T, int) NATIVE_RANK2(hipblas##U##syr2k_64, T, T, int64_t) \
    NATIVE_SYMM(hipblas##U##symm, T, int) NATIVE_SYMM(hipblas##U##symm_64, T, int64_t)         \
    NATIVE_TRMM(hipblas##U##trmm, T, int) NATIVE_TRMM(hipblas##U##trmm_64, T, int64_t)         \
    NATIVE_TRSM(hipblas##U##trsm, T, int) NATIVE_TRSM(hipblas##U##trsm_64, T, int64_t)
#define NATIVE_HERM(U, T, R)                                                                   \
    NATIVE_RANK1(hipblas##U##herk, T, R, int) NATIVE_RANK1(hipblas##U##herk_64, T, R, int64_t)   \
    NATIVE_RANK2(hipblas##U##her2k, T, R, int) NATIVE_RANK2(hipblas##U##her2k_64, T, R, int64_t) \
    NATIVE_SYMM(hipblas##U##hemm, T, int) NATIVE_SYMM(hipblas##U##hemm_64, T, int64_t)
NATIVE_TYPE(S, float)
NATIVE_TYPE(D, double)
NATIVE_TYPE(C, hipComplex)
NATIVE_TYPE(Z, hipDoubleComplex)
NATIVE_HERM(C, hipComplex, float)
NATIVE_HERM(Z, hipDoubleComplex, double)

#ifndef MOCK_LEVEL3_NATIVES_ONLY
// ---- the Level-3 entries of the libgemmul8 C ABI
namespace {
// a scalar of the call's element type, or of its real type (HERK's alpha and beta, HER2K's beta)
std::string V(int dtype, bool real, const void* s) {
    switch (dtype) {
    case GEMMUL8_S: return V((const float*)s);
    case GEMMUL8_D: return V((const double*)s);
    case GEMMUL8_C: return real ? V((const float*)s) : V((const hipComplex*)s);
    default: return real ? V((const double*)s) : V((const hipDoubleComplex*)s);
    }
}
size_t pad256(size_t x) { return (x + 255) / 256 * 256; }
size_t gemm_work(int dtype, int backend, size_t m, size_t n, size_t k, unsigned N) { return gemmul8_work_size(dtype >= 2, backend, m, n, k, N, 0, 0, nullptr, nullptr); }
int finish(void* work, size_t entitled) {
    if (work) ((volatile char*)work)[entitled - 1] = 0x33;
    const char* rc = std::getenv("MOCK_LEVEL3_RC");
    return rc ? std::atoi(rc) : GEMMUL8_OK;
}
const char* nn(const void* p) { return p ? "non-null" : "null"; }
int rank1(const char* name, void* stream, int dtype, int backend, int uplo, int trans, size_t n, size_t k, const void* alpha, bool real, const void* A,
          size_t lda, const void* beta, void* C, size_t ldc, unsigned N, int fast, void* work, double* timers) {
    std::printf("abi %s stream=%s dtype=%d backend=%d uplo=%d trans=%d n=%zu k=%zu alpha=%s A=%s lda=%zu beta=%s C=%s ldc=%zu N=%u fastmode=%d work=%s timers=%s\n",
                name, nn(stream), dtype, backend, uplo, trans, n, k, S(V(dtype, real, alpha)), S(P(A)), lda, S(V(dtype, real, beta)), S(P(C)), ldc, N, fast,
                nn(work), nn(timers));
    return finish(work, gemm_work(dtype, backend, n, n, k, N));
}
int rank2(const char* name, size_t kw, void* stream, int dtype, int backend, int uplo, int trans, size_t n, size_t k, const void* alpha, const void* A,
          size_t lda, const void* B, size_t ldb, const void* beta, bool real_beta, void* C, size_t ldc, unsigned N, int fast, void* work, double* timers) {
    std::printf("abi %s stream=%s dtype=%d backend=%d uplo=%d trans=%d n=%zu k=%zu alpha=%s A=%s lda=%zu B=%s ldb=%zu beta=%s C=%s ldc=%zu N=%u fastmode=%d "
                "work=%s timers=%s\n", name, nn(stream), dtype, backend, uplo, trans, n, k, S(V(dtype, false, alpha)), S(P(A)), lda, S(P(B)), ldb,
                S(V(dtype, real_beta, beta)), S(P(C)), ldc, N, fast, nn(work), nn(timers));
    return finish(work, gemm_work(dtype, backend, n, n, kw, N));
}
int symm(const char* name, void* stream, int dtype, int backend, int side, int uplo, size_t m, size_t n, const void* alpha, const void* A, size_t lda,
         const void* B, size_t ldb, const void* beta, void* C, size_t ldc, unsigned N, int fast, void* work, double* timers) {
    std::printf("abi %s stream=%s dtype=%d backend=%d side=%d uplo=%d m=%zu n=%zu alpha=%s A=%s lda=%zu B=%s ldb=%zu beta=%s C=%s ldc=%zu N=%u fastmode=%d "
                "work=%s timers=%s\n", name, nn(stream), dtype, backend, side, uplo, m, n, S(V(dtype, false, alpha)), S(P(A)), lda, S(P(B)), ldb,
                S(V(dtype, false, beta)), S(P(C)), ldc, N, fast, nn(work), nn(timers));
    return finish(work, gemm_work(dtype, backend, m, n, side == HIPBLAS_SIDE_LEFT ? m : n, N));
}
}  // namespace
EXPORT int gemmul8_set_nonfinite_mode(int mode) {
    std::printf("abi gemmul8_set_nonfinite_mode mode=%d\n", mode);
    return 0;
}
EXPORT int gemmul8_syrk(void* stream, int dtype, int backend, int uplo, int trans, size_t n, size_t k, const void* alpha, const void* A, size_t lda,
                        const void* beta, void* C, size_t ldc, unsigned N, int fast, void* work, double* timers) {
    return rank1("gemmul8_syrk", stream, dtype, backend, uplo, trans, n, k, alpha, false, A, lda, beta, C, ldc, N, fast, work, timers);
}
EXPORT int gemmul8_herk(void* stream, int dtype, int backend, int uplo, int trans, size_t n, size_t k, const void* alpha, const void* A, size_t lda,
                        const void* beta, void* C, size_t ldc, unsigned N, int fast, void* work, double* timers) {
    return rank1("gemmul8_herk", stream, dtype, backend, uplo, trans, n, k, alpha, true, A, lda, beta, C, ldc, N, fast, work, timers);
}
EXPORT int gemmul8_syr2k(void* stream, int dtype, int backend, int uplo, int trans, size_t n, size_t k, const void* alpha, const void* A, size_t lda,
                         const void* B, size_t ldb, const void* beta, void* C, size_t ldc, unsigned N, int fast, void* work, double* timers) {
    return rank2("gemmul8_syr2k", 2 * pad256(k), stream, dtype, backend, uplo, trans, n, k, alpha, A, lda, B, ldb, beta, false, C, ldc, N, fast, work, timers);
}
EXPORT int gemmul8_her2k(void* stream, int dtype, int backend, int uplo, int trans, size_t n, size_t k, const void* alpha, const void* A, size_t lda,
                         const void* B, size_t ldb, const void* beta, void* C, size_t ldc, unsigned N, int fast, void* work, double* timers) {
    return rank2("gemmul8_her2k", k, stream, dtype, backend, uplo, trans, n, k, alpha, A, lda, B, ldb, beta, true, C, ldc, N, fast, work, timers);
}
EXPORT int gemmul8_symm(void* stream, int dtype, int backend, int side, int uplo, size_t m, size_t n, const void* alpha, const void* A, size_t lda,
                        const void* B, size_t ldb, const void* beta, void* C, size_t ldc, unsigned N, int fast, void* work, double* timers) {
    return symm("gemmul8_symm", stream, dtype, backend, side, uplo, m, n, alpha, A, lda, B, ldb, beta, C, ldc, N, fast, work, timers);
}
EXPORT int gemmul8_hemm(void* stream, int dtype, int backend, int side, int uplo, size_t m, size_t n, const void* alpha, const void* A, size_t lda,
                        const void* B, size_t ldb, const void* beta, void* C, size_t ldc, unsigned N, int fast, void* work, double* timers) {
    return symm("gemmul8_hemm", stream, dtype, backend, side, uplo, m, n, alpha, A, lda, B, ldb, beta, C, ldc, N, fast, work, timers);
}
EXPORT int gemmul8_trmm(void* stream, int dtype, int backend, int side, int uplo, int trans, int diag, size_t m, size_t n, const void* alpha, const void* A,
                        size_t lda, const void* B, size_t ldb, void* C, size_t ldc, unsigned N, int fast, void* work, double* timers) {
    std::printf("abi gemmul8_trmm stream=%s dtype=%d backend=%d side=%d uplo=%d trans=%d diag=%d m=%zu n=%zu alpha=%s A=%s lda=%zu B=%s ldb=%zu C=%s ldc=%zu N=%u "
                "fastmode=%d work=%s timers=%s\n", nn(stream), dtype, backend, side, uplo, trans, diag, m, n, S(V(dtype, false, alpha)), S(P(A)), lda, S(P(B)),
                ldb, S(P(C)), ldc, N, fast, nn(work), nn(timers));
    return finish(work, gemm_work(dtype, backend, m, n, side == HIPBLAS_SIDE_LEFT ? m : n, N));
}
// not the GEMM's size on purpose: a hook that sized a TRSM workspace as the other side routines' would come out short
EXPORT size_t gemmul8_trsm_work_size(int cplx, int backend, int side, size_t m, size_t n, unsigned N) {
    return gemmul8_work_size(cplx, backend, m, n, side == HIPBLAS_SIDE_LEFT ? m : n, N, 0, 0, nullptr, nullptr) + 4096 + 64;
}
EXPORT int gemmul8_trsm(void* stream, int dtype, int backend, int side, int uplo, int trans, int diag, size_t m, size_t n, const void* alpha, const void* A,
                        size_t lda, void* B, size_t ldb, unsigned N, int fast, void* work, double* timers) {
    std::printf("abi gemmul8_trsm stream=%s dtype=%d backend=%d side=%d uplo=%d trans=%d diag=%d m=%zu n=%zu alpha=%s A=%s lda=%zu B=%s ldb=%zu N=%u fastmode=%d "
                "work=%s timers=%s\n", nn(stream), dtype, backend, side, uplo, trans, diag, m, n, S(V(dtype, false, alpha)), S(P(A)), lda, S(P(B)), ldb, N, fast,
                nn(work), nn(timers));
    return finish(work, gemmul8_trsm_work_size(dtype >= 2, backend, side, m, n, N));
}
#endif
