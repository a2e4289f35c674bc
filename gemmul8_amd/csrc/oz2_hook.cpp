// Drop-in hipBLAS / hipBLASLt / rocBLAS hook (LD_PRELOAD): the GEMM entry points below are interposed and routed to the Ozaki-II emulation
// (C ABI, gemmul8_c.h) according to the GEMMUL8_* environment variables; every call the environment does not select, and every call outside
// what the emulator accepts, goes to the real routine: the next definition in the search order, or the library's already-mapped copy (real()).
// One translation unit without kernels; it calls no BLAS routine itself.  Built twice: into libgemmul8.so, and with -DOZ2_HOOK_SHIM as
// libgemmul8_preload.so (see abi()).
//
// Interposed symbols                                                       beyond the reference (src/hook.cu:846-1055)?
//   hipblas{S,D,C,Z}gemm, hipblasGemmEx, hipblasDestroy                     no: m|n|k <= 0 -> SUCCESS, null A/B/C -> INVALID_VALUE (hook.cu:616-617)
//   hipblas{S,D,C,Z}gemm_64, hipblasGemmEx_64,                              yes (ROCm 7 ILP64 / WithFlags twins): the same contract; emulated when every
//     hipblasGemmExWithFlags, hipblasGemmExWithFlags_64                       dimension fits an int, native otherwise
//   hipblas{S,D,C,Z}gemmStridedBatched, hipblasGemmStridedBatchedEx         yes (torch.bmm): no early out, degenerate calls are the native routine's
//   hipblas{S,D,C,Z}gemmBatched(_64), hipblasGemmBatchedEx(_64),            yes (pointer arrays in device memory): one set of launches through gemmul8_gemm_batched_ptr, the
//     hipblasGemmBatchedExWithFlags(_64)                                      arrays are never read on the host; no per-item fallback, see emulate_batch_ptr
//   hipblas{S,D,C,Z}syrk(_64), hipblas{C,Z}herk(_64),                       yes: the Level-3 routines beyond GEMM, each through its gemmul8_* entry point (INT8 backend only), everything
//     hipblas{S,D,C,Z}syr2k(_64), hipblas{C,Z}her2k(_64),                     the emulation does not take is the native routine's; one gate for the eight, see try_level3:
//     hipblas{S,D,C,Z}symm(_64), hipblas{C,Z}hemm(_64),                       one triangle of C for the rank-k four (k <= 2^17, SYR2K: 2^16), one triangle of A read in place for
//     hipblas{S,D,C,Z}trmm(_64), hipblas{S,D,C,Z}trsm(_64)                    SYMM / HEMM / TRMM (ROCm 7's out-of-place signature) / TRSM (in place on B), order of A <= 2^17
//   hipblasLtMatmul, hipblasLtDestroy                                       yes (PyTorch's float32 matmuls): the plain case only, see lt_try
//   hipblasLtMatrixLayoutCreate / SetAttribute / Destroy                    yes: record what a layout holds (hipBLASLt cannot be asked)
//   rocblas_{s,d,c,z}gemm, rocblas_{s,d,c,z}gemm_strided_batched,           yes, only with GEMMUL8_HOOK_ROCBLAS=1: applications that call rocBLAS directly
//     rocblas_gemm_ex (in-place form), rocblas_destroy_handle                 (HPL-style codes)
//   rocblas_{s,d,c,z}gemm_batched(_64), rocblas_gemm_batched_ex (in place)  yes, only with GEMMUL8_HOOK_ROCBLAS=1: the pointer-array forms, as for hipBLAS
//   rocblas_internal_gemm_template<T> / _64<T>, T = float, double,          yes, only with GEMMUL8_HOOK_ROCBLAS=1 and a tested rocBLAS release: rocSOLVER's
//     rocblas_complex_num<float / double> (eight mangled names)               trailing updates (INTEGRATION.md "What the hook reaches")
//   gemmul8_hook_would_emulate, gemmul8_hook_rocblas_version_tested         this project's own queries (no interposition)
//
// Environment                      read        meaning                                                      hook.cu:170-227,232-310
//   GEMMUL8_NUM_MOD_{S,D,C,Z}      per call    emulate when 2 <= N <= 13 (S,C) / 20 (D,Z); otherwise native
//   GEMMUL8_FASTMODE_{S,D,C,Z}     per call    "1" = fast mode, default accurate
//   GEMMUL8_BACKEND                per call    0|INT8 (default) / 1|FP8
//   GEMMUL8_SKIP_SCALE_{A,B}       per call    "1" = keep the quantised operand + shifts between calls (pointer identity)
//   GEMMUL8_MAX_{M,N,K}, GEMMUL8_MAX_NUM_MOD, GEMMUL8_MAXWS_BACKEND
//                                  once        workspace pre-sizing, applied when a SKIP_SCALE switch is on (hook.cu:232-281,656-662)
//  the rest is this build's only:
//   GEMMUL8_FP8_BOUND, GEMMUL8_NONFINITE
//                                  once        `reference` / `ieee`: gemmul8_set_fp8_bound_mode / gemmul8_set_nonfinite_mode (init_max_workspace); under `ieee` the Level-3
//                                              routines beyond GEMM are not emulated (try_level3)
//   GEMMUL8_MIN_FLOPS              per call    unset or 0 = emulate every selected call (the reference's behaviour); `auto` = a fitted cost model decides
//                                              per call (below_floor; level3_below_floor); a number = floor on 2*m*n*k.  The first call a floor declines is logged once.
//   GEMMUL8_DIST                   per call    blocks | moduli | fp64sum: shard every emulated GEMM over the ranks of an SPMD job (try_dist)
//   GEMMUL8_BATCH_FUSED, GEMMUL8_BATCH_WORKSPACE_MB, GEMMUL8_BATCH_STREAMS
//                                  per call    strided batches: one set of launches (default) in chunks of the given size, or lanes (emulate_batch)
//                                              pointer-array batches: one set of launches in chunks of the given size; GEMMUL8_BATCH_FUSED=0 (or GEMMUL8_DIST)
//                                              = the native routine, said once (emulate_batch_ptr: the lanes would walk item addresses on the host)
//   GEMMUL8_HOOK_ROCBLAS           per call    "1" = the rocBLAS entry points above act
//   GEMMUL8_ROCBLAS_ABI_UNCHECKED  once        "1" = interpose the internal template on any rocBLAS release (rocblas_internal_abi_ok)
//   GEMMUL8_HOOK_STATS             once        "1" = print at exit how many GEMM calls / flops were emulated and how many went native (count_call);
//                                              a line each for hipblas{S,D,C,Z}syrk, hipblas{C,Z}herk, hipblas{S,D,C,Z}syr2k, hipblas{C,Z}her2k, hipblas{S,D,C,Z}symm,
//                                              hipblas{C,Z}hemm, hipblas{S,D,C,Z}trmm and hipblas{S,D,C,Z}trsm when one was seen
//   GEMMUL8_HOOK_VERBOSE           per call    "1" = say why a hipblasLtMatmul call was left to the native routine
//
// Per-handle state under a mutex: three grow-only stream-ordered buffers (hipMallocAsync / hipFreeAsync), event hand-off when the handle's
// stream changes, skip-scaling cache (hook.cu:70-162,331-374,684-727); hipblasDestroy frees the state first (hook.cu:846-856).
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hipblas/hipblas.h>
#include <hipblaslt/hipblaslt.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/gemmul8_c.h"
#include "../../include/gemmul8_dist.h"

// The C ABI the hook calls: X(name, attribute) for gemmul8_<name>.  Everything that concerns these symbols is generated from this list.
// `weak` marks an entry a library linked with this file may lack (tests/sanitize/mock_gpu.cpp has no gemmul8_set_nonfinite_mode: the mode
// then stays 0 -- and no gemmul8_syrk / gemmul8_herk / gemmul8_syr2k / gemmul8_her2k / gemmul8_symm / gemmul8_hemm / gemmul8_trmm / gemmul8_trsm / gemmul8_gemm_batched_ptr: every such call then goes to the native routine); the shim, which binds to this
// project's own libgemmul8.so, requires every entry.
#define OZ2_ABI(X)                                                                                          \
    X(work_size, ) X(gemm, ) X(work_size_batched, ) X(gemm_batched, ) X(add_row_bias, ) X(set_fp8_bound_mode, ) \
    X(comm_rccl_from_env, ) X(dist_create, ) X(dist_gemm, ) X(dist_allgather_c, ) X(dist_destroy, )             \
    X(set_nonfinite_mode, __attribute__((weak))) X(syrk, __attribute__((weak))) X(herk, __attribute__((weak))) \
    X(syr2k, __attribute__((weak))) X(symm, __attribute__((weak))) X(hemm, __attribute__((weak))) X(her2k, __attribute__((weak))) \
    X(trmm, __attribute__((weak))) X(trsm, __attribute__((weak))) X(trsm_work_size, __attribute__((weak))) \
    X(gemm_batched_ptr, __attribute__((weak)))
#ifndef OZ2_HOOK_SHIM
#define X(name, attr) extern "C" attr decltype(::gemmul8_##name) gemmul8_##name;
OZ2_ABI(X)
#undef X
#endif
// the rocBLAS routines the hook calls without defining them (rocblas_status / rocblas_handle as plain int / void*, see the rocBLAS entry
// points below); declared for decltype only, never referenced
extern "C" int rocblas_get_stream(void*, hipStream_t*);
extern "C" int rocblas_get_version_string_size(size_t*);
extern "C" int rocblas_get_version_string(char*, size_t);

namespace {

// ---- libraries: the real routines and the C ABI
// an already-mapped library whose path contains `needle`, found in /proc/self/maps and re-opened (never loaded) with the given scope
void* mapped_library(const char* needle, int scope) {
    void* r = nullptr;
    if (FILE* f = std::fopen("/proc/self/maps", "r")) {
        char line[1024];
        while (std::fgets(line, sizeof line, f)) {
            if (!std::strstr(line, needle)) continue;
            char* path = std::strchr(line, '/');
            if (!path) continue;
            path[std::strcspn(path, "\n")] = 0;
            r = dlopen(path, RTLD_NOW | scope | RTLD_NOLOAD);
            if (r) break;
        }
        std::fclose(f);
    }
    return r;
}
// the already-mapped copy of the library an interposed name belongs to (each looked up once, on first need)
void* home_library(const char* name) {
    if (std::strncmp(name, "hipblasLt", 9) == 0) {
        static void* const h = mapped_library("libhipblaslt.so", RTLD_LOCAL);
        return h;
    }
    if (std::strstr(name, "rocblas_")) {  // the C entry points and the mangled rocblas_internal_gemm_template names
        static void* const h = mapped_library("librocblas.so", RTLD_LOCAL);
        return h;
    }
    static void* const h = mapped_library("libhipblas.so", RTLD_LOCAL);  // not libhipblaslt
    return h;
}
// The real routine behind an interposed name (Fn = decltype(&NAME): the hook defines a function of exactly that name and type): the next
// definition in the global search order, or -- when the host loaded the library privately (Python extension modules are dlopen'ed
// RTLD_LOCAL) -- the one in the library's mapped copy.
template <typename Fn> Fn real(const char* name) {
    void* f = dlsym(RTLD_NEXT, name);
    if (!f)
        if (void* lib = home_library(name)) f = dlsym(lib, name);
    return reinterpret_cast<Fn>(f);
}
#define OZ2_REAL(NAME) static const auto real_ = real<decltype(&NAME)>(#NAME)
// every pass-through runs inside a NativeScope (below)
#define OZ2_NATIVE(NAME, MISSING, ...) \
    OZ2_REAL(NAME);                    \
    NativeScope ns_;                   \
    return real_ ? real_(__VA_ARGS__) : MISSING

struct Abi {
#define X(name, attr) decltype(&::gemmul8_##name) name = nullptr;
    OZ2_ABI(X)
#undef X
};
#ifdef OZ2_HOOK_SHIM
// Preload shim for hosts that load their HIP runtime late and privately (Python/PyTorch): this library contains no device
// code (so nothing registers with the HIP runtime when the loader maps it at process start) and binds to libgemmul8.so --
// which does -- on the first intercepted call: by then the host's libamdhip64 is mapped; it is promoted to the global symbol
// scope, then libgemmul8.so (found next to this file) is opened and the C-ABI entry points the hook needs are resolved.
const Abi& abi() {
    static const Abi a = [] {
        Abi r;
        (void)mapped_library("libamdhip64", RTLD_GLOBAL);  // promote the HIP runtime the process already uses
        Dl_info info;
        std::string dir = ".";
        if (dladdr((const void*)&abi, &info) && info.dli_fname) {
            dir = info.dli_fname;
            const size_t slash = dir.rfind('/');
            dir = slash == std::string::npos ? "." : dir.substr(0, slash);
        }
        void* h = dlopen((dir + "/libgemmul8.so").c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) {
            std::fprintf(stderr, "[GEMMUL8 HOOK] cannot open %s/libgemmul8.so: %s\n", dir.c_str(), dlerror());
            std::abort();
        }
#define X(name, attr)                                                                                                \
    if (!(r.name = (decltype(r.name))dlsym(h, "gemmul8_" #name))) {                                                  \
        std::fprintf(stderr, "[GEMMUL8 HOOK] libgemmul8.so lacks the C ABI entry point gemmul8_" #name "\n");        \
        std::abort();                                                                                                \
    }
        OZ2_ABI(X)
#undef X
        return r;
    }();
    return a;
}
#else
const Abi& abi() {
    static const Abi a = {
#define X(name, attr) &::gemmul8_##name,
        OZ2_ABI(X)
#undef X
    };
    return a;
}
#endif

struct Cache {  // what the quantised planes in workA/workB currently hold
    bool valid = false;
    unsigned num_moduli = 0;
    int op_A = 0, op_B = 0;
    size_t m = 0, n = 0, k = 0, lda = 0, ldb = 0;
    const void *A = nullptr, *B = nullptr;
    void *workA = nullptr, *workB = nullptr;
    int dtype = -1, backend = 0;
    bool fastmode = false;
    bool enA = false, enB = false;  // the skip switches move the workspace carving (extra bound plane): part of the key
};

struct Buffer {
    void* ptr = nullptr;
    size_t size = 0;
};

// side lane of a batched call: its own stream, join event and single work buffer (see emulate_batch)
struct BatchLane {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    Buffer w;
};
constexpr int kMaxBatchLanes = 8;

struct HandleState {
    std::mutex mtx;
    Buffer wA, wB, wC;
    Cache last;
    hipStream_t last_stream = nullptr;
    hipEvent_t last_event = nullptr;
    bool have_stream = false;
    bool is_lt = false;  // the key is a hipblasLtHandle_t: it has no stream of its own and must never reach hipblasGetStream
    BatchLane lanes[kMaxBatchLanes];  // lane 0 unused (= the handle's stream and buffers)
    hipEvent_t fork = nullptr;
};

std::mutex g_map_mtx;
std::unordered_map<hipblasHandle_t, std::shared_ptr<HandleState>> g_map;

std::shared_ptr<HandleState> state_of(hipblasHandle_t h) {
    std::lock_guard<std::mutex> g(g_map_mtx);
    auto& p = g_map[h];
    if (!p) p = std::make_shared<HandleState>();
    return p;
}

bool env_one(const char* name) {
    const char* s = std::getenv(name);
    return s && std::strcmp(s, "1") == 0;
}
unsigned long long env_u64(const char* name, unsigned long long def) {
    const char* s = std::getenv(name);
    if (!s || !*s) return def;
    char* end = nullptr;
    const unsigned long long v = std::strtoull(s, &end, 10);
    return (end == s) ? def : v;
}
int env_backend(const char* name, int def, bool allow_both) {
    const char* s = std::getenv(name);
    if (!s) return def;
    if (!std::strcmp(s, "0") || !std::strcmp(s, "INT8")) return 0;
    if (!std::strcmp(s, "1") || !std::strcmp(s, "FP8")) return 1;
    if (allow_both && (!std::strcmp(s, "2") || !std::strcmp(s, "BOTH"))) return 2;
    return def;
}

// ---- types, calls and what the environment selects for them
struct TypeInfo {  // indexed by GEMMUL8_{S,D,C,Z}
    const char* nmod;
    const char* fast;
    unsigned max_moduli;
    bool cplx;
    size_t elem;  // bytes
    hipDataType hip_type;
    hipblasComputeType_t compute;
    int rocblas_type;  // rocblas_datatype_{f32,f64}_{r,c}
};
const TypeInfo kTypes[4] = {
    {"GEMMUL8_NUM_MOD_S", "GEMMUL8_FASTMODE_S", 13u, false, 4, HIP_R_32F, HIPBLAS_COMPUTE_32F, 151},
    {"GEMMUL8_NUM_MOD_D", "GEMMUL8_FASTMODE_D", 20u, false, 8, HIP_R_64F, HIPBLAS_COMPUTE_64F, 152},
    {"GEMMUL8_NUM_MOD_C", "GEMMUL8_FASTMODE_C", 13u, true, 8, HIP_C_32F, HIPBLAS_COMPUTE_32F, 154},
    {"GEMMUL8_NUM_MOD_Z", "GEMMUL8_FASTMODE_Z", 20u, true, 16, HIP_C_64F, HIPBLAS_COMPUTE_64F, 155},
};
// GEMMUL8_{S,D,C,Z} for a hipDataType (an Lt layout's type included) / a rocblas_datatype code, -1 for every other type
int dtype_of(int hip_type) {
    for (int d = 0; d < 4; ++d)
        if ((int)kTypes[d].hip_type == hip_type) return d;
    return -1;
}
int dtype_of_rocblas(int code) {
    for (int d = 0; d < 4; ++d)
        if (kTypes[d].rocblas_type == code) return d;
    return -1;
}
// the *GemmEx forms: same (computeType, A/B/C type) dispatch as hook.cu:961-1030
int dtype_of(hipDataType aType, hipDataType bType, hipDataType cType, hipblasComputeType_t computeType) {
    const int d = (aType == bType && bType == cType) ? dtype_of((int)aType) : -1;
    return d >= 0 && kTypes[d].compute == computeType ? d : -1;
}

// One GEMM (batch == 1) or one strided batch as the emulator takes it: int dimensions, strides in elements
struct GemmCall {
    int dtype;
    size_t elem;  // bytes
    hipblasOperation_t ta, tb;
    int m, n, k;
    const void *alpha, *A;
    int lda;
    long long sa;
    const void* B;
    int ldb;
    long long sb;
    const void* beta;
    void* C;
    int ldc;
    long long sc;
    int batch;
};
// false = not a call the emulator can be asked about: not an S/D/C/Z type, an empty product or batch, a null matrix, or a dimension an
// int cannot hold (the ILP64 forms; the reference's CUDA-side hook predates them)
bool gemm_call(GemmCall* c, int dtype, int ta, int tb, int64_t m, int64_t n, int64_t k, const void* alpha, const void* A, int64_t lda, long long sa,
               const void* B, int64_t ldb, long long sb, const void* beta, void* C, int64_t ldc, long long sc, int64_t batch = 1) {
    const int64_t lim = 2147483647;
    if (dtype < 0 || m <= 0 || n <= 0 || k <= 0 || batch <= 0 || !A || !B || !C) return false;
    if (m > lim || n > lim || k > lim || lda > lim || ldb > lim || ldc > lim || batch > lim) return false;
    *c = GemmCall{dtype, kTypes[dtype].elem, (hipblasOperation_t)ta, (hipblasOperation_t)tb, (int)m, (int)n, (int)k, alpha, A, (int)lda, sa, B, (int)ldb, sb,
                  beta, C, (int)ldc, sc, (int)batch};
    return true;
}

struct Selection { unsigned N; bool fast; int backend; bool enA, enB; };
// what the environment asks for a type, read anew on every call; false = the moduli count does not select emulation
bool selection_from_env(int dtype, Selection* s) {
    const TypeInfo& ti = kTypes[dtype];
    *s = Selection{(unsigned)env_u64(ti.nmod, 0), env_one(ti.fast), env_backend("GEMMUL8_BACKEND", 0, false), env_one("GEMMUL8_SKIP_SCALE_A"),
                   env_one("GEMMUL8_SKIP_SCALE_B")};
    return s->N >= 2u && s->N <= ti.max_moduli;
}
// the emulator's k range (gemmul8_gemm / gemmul8_gemm_batched return GEMMUL8_E_ARG beyond it)
constexpr int kMaxK = 1 << 17, kMaxKFp8 = 65536;
bool k_in_range(const GemmCall& c, const Selection& s) { return c.k <= (s.backend == GEMMUL8_FP8 ? kMaxKFp8 : kMaxK); }

// GEMMUL8_NONFINITE=ieee, read once.  Kept here and not asked of the library: one linked with this file may lack gemmul8_set_nonfinite_mode.
bool nonfinite_ieee() {
    static const bool on = [] {
        const char* nf = std::getenv("GEMMUL8_NONFINITE");
        return nf && !std::strcmp(nf, "ieee");
    }();
    return on;
}

// process-wide workspace floor, computed once (hook.cu:232-281)
size_t g_maxA = 0, g_maxB = 0, g_maxC = 0;
std::once_flag g_max_once;
void init_max_workspace() {
    std::call_once(g_max_once, [] {
        // GEMMUL8_FP8_BOUND=reference (this build only): the reference's (k+1)*2^-24 inflation of the FP8 bound GEMM instead of the
        // engine-safe default (include/gemmul8_c.h, gemmul8_set_fp8_bound_mode)
        if (const char* fb = std::getenv("GEMMUL8_FP8_BOUND"))
            if (!std::strcmp(fb, "reference")) (void)abi().set_fp8_bound_mode(1);
        // GEMMUL8_NONFINITE=ieee: BLAS-like NaN / Inf propagation (include/gemmul8_c.h, gemmul8_set_nonfinite_mode); unset or `reference`: mode 0.
        // Not applied to the calls the multi-GPU plans take (GEMMUL8_DIST).
        // The rank-k entry points have no mode 1: their calls stay on the native routine under `ieee` (try_level3).
        if (const char* nf = std::getenv("GEMMUL8_NONFINITE"); nf && *nf) {
            if (nonfinite_ieee()) {
                if (auto set = abi().set_nonfinite_mode) (void)set(1);
            } else if (std::strcmp(nf, "reference")) {
                std::fprintf(stderr, "[GEMMUL8 HOOK] GEMMUL8_NONFINITE=%s not understood (ieee | reference): non-finite mode 0\n", nf);
            }
        }
        const size_t mm = env_u64("GEMMUL8_MAX_M", 0), mn = env_u64("GEMMUL8_MAX_N", 0), mk = env_u64("GEMMUL8_MAX_K", 0);
        const unsigned mmod = (unsigned)env_u64("GEMMUL8_MAX_NUM_MOD", 2);
        const bool cplx = env_u64("GEMMUL8_NUM_MOD_Z", 0) > 0 || env_u64("GEMMUL8_NUM_MOD_C", 0) > 0;
        const int which = env_backend("GEMMUL8_MAXWS_BACKEND", 0, true);
        for (int be = 0; be < 2; ++be) {
            if (!(which == be || which == 2)) continue;
            if (mmod < 2 || mmod > 20) continue;
            size_t wa = 0, wb = 0;
            const size_t w = abi().work_size(cplx, be, mm, mn, mk, mmod, 1, 1, &wa, &wb);
            g_maxA = std::max(g_maxA, wa);
            g_maxB = std::max(g_maxB, wb);
            g_maxC = std::max(g_maxC, w > wa + wb ? w - wa - wb : 0);
        }
    });
}

hipblasStatus_t grow(Buffer& b, size_t need, hipStream_t stream, const char* tag) {
    if (need == 0 || (b.ptr && b.size >= need)) return HIPBLAS_STATUS_SUCCESS;
    if (b.ptr) {
        const hipError_t e = hipFreeAsync(b.ptr, stream);
        if (e != hipSuccess) {
            std::fprintf(stderr, "[GEMMUL8 HOOK] hipFreeAsync failed for %s (%s)\n", tag, hipGetErrorString(e));
            return HIPBLAS_STATUS_INTERNAL_ERROR;
        }
        b.ptr = nullptr;
        b.size = 0;
    }
    void* p = nullptr;
    const hipError_t e = hipMallocAsync(&p, need, stream);
    if (e != hipSuccess) {
        std::fprintf(stderr, "[GEMMUL8 HOOK] hipMallocAsync failed for %s size %zu bytes (%s)\n", tag, need, hipGetErrorString(e));
        return HIPBLAS_STATUS_ALLOC_FAILED;
    }
    b.ptr = p;
    b.size = need;
    return HIPBLAS_STATUS_SUCCESS;
}

hipStream_t handle_stream(hipblasHandle_t h, hipblasStatus_t* st) {
    static const auto fn = real<decltype(&hipblasGetStream)>("hipblasGetStream");
    hipStream_t s = nullptr;
    *st = fn ? fn(h, &s) : HIPBLAS_STATUS_NOT_INITIALIZED;
    return s;
}

// order work on the new stream after everything queued on the previous one (hook.cu:141-162)
hipblasStatus_t order_streams(HandleState& st, hipStream_t cur) {
    if (!st.have_stream) {
        st.last_stream = cur;
        st.have_stream = true;
        return HIPBLAS_STATUS_SUCCESS;
    }
    if (st.last_stream == cur) return HIPBLAS_STATUS_SUCCESS;
    if (!st.last_event && hipEventCreateWithFlags(&st.last_event, hipEventDisableTiming) != hipSuccess) return HIPBLAS_STATUS_INTERNAL_ERROR;
    if (hipEventRecord(st.last_event, st.last_stream) != hipSuccess) return HIPBLAS_STATUS_INTERNAL_ERROR;
    if (hipStreamWaitEvent(cur, st.last_event, 0) != hipSuccess) return HIPBLAS_STATUS_INTERNAL_ERROR;
    st.last_stream = cur;
    return HIPBLAS_STATUS_SUCCESS;
}

// The handle's state, locked for as long as this object lives, and the stream the call runs on, ordered after the handle's previous one
// (st != SUCCESS: neither).  explicit_stream: hipblasLtMatmul and the rocBLAS entry points carry / look up their stream themselves; such
// a handle is no hipblasHandle_t and is marked so that it never reaches hipblasGetStream (release_state).
struct LockedState {
    std::shared_ptr<HandleState> sp;
    std::unique_lock<std::mutex> lk;
    hipStream_t stream = nullptr;
    hipblasStatus_t st = HIPBLAS_STATUS_SUCCESS;
};
LockedState lock_ordered(hipblasHandle_t handle, const hipStream_t* explicit_stream) {
    LockedState l;
    l.sp = state_of(handle);
    l.lk = std::unique_lock<std::mutex>(l.sp->mtx);
    if (explicit_stream) l.sp->is_lt = true;
    init_max_workspace();
    l.stream = explicit_stream ? *explicit_stream : handle_stream(handle, &l.st);
    if (l.st == HIPBLAS_STATUS_SUCCESS) l.st = order_streams(*l.sp, l.stream);
    return l;
}

// ---- GEMMUL8_DIST = blocks | moduli | fp64sum (not in the reference, which is single-GPU): an SPMD application -- every rank of a
// torchrun / mpirun job issuing the SAME GEMM calls on replicated operands, RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in its
// environment -- gets each emulated GEMM sharded over the ranks' GPUs by the plans of include/gemmul8_dist.h; the result is
// all-gathered so that every rank ends up with the full C, as it would without the hook.  One RCCL communicator per process, a
// small cache of plans keyed by the call's shape (a plan owns its workspaces).
struct DistKey {
    int kind, dtype, backend, ta, tb, fast;
    size_t m, n, k;
    unsigned N;
    bool operator==(const DistKey& o) const {
        return kind == o.kind && dtype == o.dtype && backend == o.backend && ta == o.ta && tb == o.tb && fast == o.fast && m == o.m && n == o.n &&
               k == o.k && N == o.N;
    }
};
// One communicator and one plan cache serve every handle and stream of the process, so the sharded calls are CHAINED: each call
// records `tail` on its stream when its last operation is enqueued and the next call -- on whatever stream -- first makes its
// stream wait for it.  Two handles / streams issuing same-shape GEMMs therefore never overlap on a plan's workspaces, and the RCCL
// operations of the one communicator execute in the order they were enqueued (mtx gives the enqueue order; every rank of an SPMD
// job issues the same sequence).
struct DistState {
    std::mutex mtx;
    gemmul8_comm* comm = nullptr;
    bool failed = false;
    std::vector<std::pair<DistKey, gemmul8_dist_plan*>> plans;  // most recently used last; at most 8
    hipEvent_t tail = nullptr;      // completion of the most recent sharded call
    hipStream_t tail_stream = nullptr;
    bool have_tail = false;
};
DistState g_dist;

int dist_kind_from_env() {
    const char* s = std::getenv("GEMMUL8_DIST");
    if (!s || !*s || !std::strcmp(s, "0")) return -1;
    if (!std::strcmp(s, "moduli")) return GEMMUL8_DIST_MODULI;
    if (!std::strcmp(s, "fp64sum")) return GEMMUL8_DIST_MODULI_FP64SUM;
    return GEMMUL8_DIST_BLOCKS;  // "1", "blocks"
}

// returns true when the sharded path took the call (status in *status); false -> single-GPU emulation.
// Falling back is only safe when EVERY rank takes the same decision, i.e. for reasons that are a function of the call's arguments
// and the environment (negative GEMMUL8_E_ARG / _NUM_MODULI / _UNSUPPORTED from plan creation, no communicator at all).  A
// resource failure on one rank (GEMMUL8_E_INTERNAL: allocation, transport) is reported as HIPBLAS_STATUS_INTERNAL_ERROR instead: a
// rank that silently computed alone would leave its peers waiting in a collective.
bool try_dist(int kind, const GemmCall& c, const Selection& s, hipStream_t stream, hipblasStatus_t* status) {
    std::lock_guard<std::mutex> lk(g_dist.mtx);
    if (g_dist.failed) return false;
    if (!g_dist.comm) {
        const int rc = abi().comm_rccl_from_env(&g_dist.comm);
        if (rc != 0 || !g_dist.comm) {
            // decided before any collective has been issued; ncclCommInitRank itself fails on every rank when one is missing
            std::fprintf(stderr, "[GEMMUL8 HOOK] GEMMUL8_DIST is set but no RCCL communicator could be created (status %d; RANK/WORLD_SIZE/"
                                 "MASTER_ADDR/MASTER_PORT?): single-GPU emulation\n", rc);
            g_dist.failed = true;
            return false;
        }
    }
    if (!g_dist.tail && hipEventCreateWithFlags(&g_dist.tail, hipEventDisableTiming) != hipSuccess) return *status = HIPBLAS_STATUS_INTERNAL_ERROR, true;
    // chain behind the previous sharded call (any handle, any stream)
    if (g_dist.have_tail && g_dist.tail_stream != stream && hipStreamWaitEvent(stream, g_dist.tail, 0) != hipSuccess)
        return *status = HIPBLAS_STATUS_INTERNAL_ERROR, true;
    const DistKey key{kind, c.dtype, s.backend, (int)c.ta, (int)c.tb, s.fast ? 1 : 0, (size_t)c.m, (size_t)c.n, (size_t)c.k, s.N};
    gemmul8_dist_plan* plan = nullptr;
    for (size_t i = 0; i < g_dist.plans.size(); ++i)
        if (g_dist.plans[i].first == key) {
            plan = g_dist.plans[i].second;
            std::rotate(g_dist.plans.begin() + i, g_dist.plans.begin() + i + 1, g_dist.plans.end());
            break;
        }
    if (!plan) {
        if (g_dist.plans.size() >= 8) {  // plans own workspaces of the problem's size: keep only a few
            // every earlier sharded call is an ancestor of `tail`: once it has completed no stream still uses the evicted plan
            if (g_dist.have_tail && hipEventSynchronize(g_dist.tail) != hipSuccess) (void)hipDeviceSynchronize();
            abi().dist_destroy(g_dist.plans.front().second);
            g_dist.plans.erase(g_dist.plans.begin());
        }
        const int rc = abi().dist_create(g_dist.comm, nullptr, kind, 0, c.dtype, s.backend, (int)c.ta, (int)c.tb, (size_t)c.m, (size_t)c.n, (size_t)c.k,
                                         s.N, s.fast ? 1 : 0, &plan);
        if (rc == GEMMUL8_E_INTERNAL || rc > 0 || (rc == 0 && !plan)) {
            std::fprintf(stderr, "[GEMMUL8 HOOK] GEMMUL8_DIST: creating the plan failed on this rank (status %d): returning an error (the other "
                                 "ranks are entering the collective)\n", rc);
            return *status = HIPBLAS_STATUS_INTERNAL_ERROR, true;
        }
        if (rc != 0) return false;  // a property of the arguments (outside the emulator's range): every rank declines alike
        g_dist.plans.emplace_back(key, plan);
    }
    int rc = abi().dist_gemm(plan, stream, c.alpha, c.A, (size_t)c.lda, c.B, (size_t)c.ldb, c.beta, c.C, (size_t)c.ldc);
    if (rc == 0) rc = abi().dist_allgather_c(plan, stream, c.C, (size_t)c.ldc);
    if (hipEventRecord(g_dist.tail, stream) == hipSuccess) g_dist.tail_stream = stream, g_dist.have_tail = true;
    else rc = rc ? rc : 1;
    *status = rc == 0 ? HIPBLAS_STATUS_SUCCESS : HIPBLAS_STATUS_INTERNAL_ERROR;
    return true;
}

// GEMMUL8_MIN_FLOPS (not in the reference).  A drop-in must not make an application slower by default: small products are ten
// latency-bound launches (1024^3: 21 vs 48 TFLOPS native), and what a hooked solver issues most -- trailing updates with large m = n
// and small k, panel products with one small dimension -- pays the per-output cost of the scheme (N bytes of residues written, read
// and recombined per element) without the k to amortise it (DGEMM 8192^2 x 256: 45 vs 65 TFLOPS native; x 512: 71 vs 69; x 1024:
// 107 vs 70).  With GEMMUL8_MIN_FLOPS=auto the hook therefore evaluates a fitted cost model per call and emulates only where the
// emulation is predicted to win (opt-in: the numerics of a call then depend on its shape, and the constants were fitted on one
// MI355X pool -- the default stays the reference's: every selected call is emulated):
//     emulated  t_e = c0 + (a1 + b1 N)(m + n) k + (a2 + b2 N) m n + b3 N m n k      per (type, accurate / fast), N = number of moduli
//     native    t_n = d0 + d2 m n + d3 m n k                                        per type (the library at its normal rate)
//     emulate   iff t_e <= 0.95 t_n        (a strided batch: one set of launches, so c0 / d0 once and the rest times the batch)
// Constants: tools/fit_floor.py on profiles/sweeps/r03_floor_scan_{s,d,c,z}.csv (tools/floor_scan.py: 60-68 shapes x 3 N x 2 modes
// per type against the native routine on the same box; median model error 5-7 %).  On the scanned shapes the rule emulates 31-53 of
// 180-204 cases per type and mode, lets 0-2 marginal losses through (worst 1.05x the native time, one 1.19x), and the summed time is
// within 0.3-10 % of always picking the faster of the two (always-native: +25-45 %); repeated on a second box with the final binaries
// (r03_floor_scan2_*.csv, not used for the fit) it stays within 0.4-12 % (tests/test_hook_floor.py).  The FP8 backend is priced as
// the INT8 model x a per-type factor: the median time ratio at EQUAL moduli count over the same shape classes on the round-5 kernels (FP6 operand
// planes, fused three-product tile loop; tools/fp8_factor_scan.py, profiles/sweeps/r05_fp8_factor_{s,d,c,z}.csv: 1.74 / 1.90 / 2.04 / 2.12,
// range 1.3-3.1; 2.2 for every type until round 4).
// GEMMUL8_MIN_FLOPS unset / 0 = the reference's behaviour (emulate every call); any other number is a plain floor on 2*m*n*k per call.
// GEMMUL8_HOOK_STATS=1: how much of an application's GEMM work the hook reaches (tests/test_gpu_hook_reach.py)
// A call handed to the native routine comes back through the interposed layers below it (hipblasDgemm -> rocblas_dgemm ->
// rocblas_internal_gemm_template with GEMMUL8_HOOK_ROCBLAS=1): it is the SAME call, already declined by the same rules.  Every
// pass-through runs inside a NativeScope; a hooked entry reached inside one goes straight to its real routine, uncounted.
thread_local int tl_native_depth = 0;
struct NativeScope {
    NativeScope() { ++tl_native_depth; }
    ~NativeScope() { --tl_native_depth; }
    NativeScope(const NativeScope&) = delete;
    NativeScope& operator=(const NativeScope&) = delete;
};
// ---- the Level-3 routines beyond GEMM (no counterpart in the reference): one table, one call record (Level3Call), one gate (try_level3).
// Two families.  Rank-k: one triangle of the n x n matrix C from operands with inner dimension k -- SYRK alpha A A^T + beta C, HERK alpha A A^H + beta C
// (real alpha, beta), SYR2K alpha (A B^T + B A^T) + beta C, HER2K alpha A B^H + conj(alpha) B A^H + beta C (complex alpha, real beta).  Side: B and C are
// m x n and A, of which one triangle is stored and read in place, has order ka = m (side = left) / n (right) -- SYMM / HEMM alpha A B + beta C or
// alpha B A + beta C, TRMM C = alpha op(A) B or alpha B op(A) (ROCm 7's out-of-place signature; C == B is gemmul8_trmm's contract), TRSM op(A) X = alpha B
// or X op(A) = alpha B with X over B.
enum Routine { kSYRK, kHERK, kSYR2K, kHER2K, kSYMM, kHEMM, kTRMM, kTRSM, kRoutines };  // the order of the statistics lines
enum Ops { kOpsNT, kOpsNC, kOpsNone, kOpsNTC };  // the operations a routine takes: N / T, N / C, it has no such argument, N / T / C and a diag
// kTrsmAutoMinOrder: the smallest measured order of A from which the emulated TRSM beats the native one at n = ka in float64 accurate mode
// (profiles/trsm_ab.json, tools/trsm_ab.py; INTEGRATION.md "TRSM" prints the table): DTRSM left at 14 moduli loses at 8192 x 8192 (25.1 against 19.4 ms) and
// wins at 16384 x 16384 (88.6 against 108.1 ms).  The rule asks for the order only: it also declines the right-side 8192 x 8192 row, which the emulation wins.
constexpr int kTrsmAutoMinOrder = 16384;
struct RoutineInfo {
    const char* name;    // in the notices and the statistics
    const char* tag;     // the workspace's name in grow()'s messages
    bool side;           // the family
    Ops ops;
    bool beta, B;        // the pointers required beyond alpha, A and C
    int limit;           // the largest k (rank-k) / order of A (side) the emulation takes
    int k_fold;          // rank-k: the GEMM the call amounts to is (n, n, k_fold k) -- SYR2K puts A and B side by side, hence its limit of 2^16; side: (m, n, ka)
    double floor_flops;  // GEMMUL8_MIN_FLOPS as a number: a floor on floor_flops x n (n + 1) k (rank-k) / m n ka (side), the routine's own count (HER2K's in real operations)
    int auto_min_order;  // GEMMUL8_MIN_FLOPS=auto: 0 = the GEMM model's decision for that GEMM (no scan of these routines has been fitted; SYRK / HERK, native and
                         // emulated, are both about half their GEMMs; conservative for TRMM, which does less work than its GEMM); otherwise decline below this order of A
    double stats_flops;  // GEMMUL8_HOOK_STATS: stats_flops x the same product (x 4 for complex) / 1e6, rounded down
};
const RoutineInfo kRoutine[kRoutines] = {
    {"SYRK", "workC (syrk)", false, kOpsNT, true, false, kMaxK, 1, 1.0, 0, 1.0},
    {"HERK", "workC (herk)", false, kOpsNC, true, false, kMaxK, 1, 1.0, 0, 1.0},
    {"SYR2K", "workC (syr2k)", false, kOpsNT, true, true, kMaxK / 2, 2, 2.0, 0, 2.0},
    {"HER2K", "workC (her2k)", false, kOpsNC, true, true, kMaxK, 1, 8.0, 0, 2.0},
    {"SYMM", "workC (symm)", true, kOpsNone, true, true, kMaxK, 1, 2.0, 0, 2.0},
    {"HEMM", "workC (hemm)", true, kOpsNone, true, true, kMaxK, 1, 2.0, 0, 2.0},
    {"TRMM", "workC (trmm)", true, kOpsNTC, false, true, kMaxK, 1, 1.0, 0, 1.0},
    {"TRSM", "workC (trsm)", true, kOpsNTC, false, false, kMaxK, 1, 1.0, kTrsmAutoMinOrder, 1.0},
};
// One Level-3 call as its hipBLAS entry point received it (GemmCall's role); what a routine does not have stays zero / null
struct Level3Call {
    Routine routine;
    int dtype;
    int side = 0, uplo = 0, trans = 0, diag = 0;
    int64_t m = 0, n = 0, k = 0;
    const void *alpha = nullptr, *A = nullptr;
    int64_t lda = 0;
    const void* B = nullptr;
    int64_t ldb = 0;
    const void* beta = nullptr;
    void* C = nullptr;  // the matrix written: TRSM's is hipBLAS's B
    int64_t ldc = 0;
    // the product the floor and the statistics scale: n (n + 1) k / m n ka
    double flops() const {
        const double dm = (double)m, dn = (double)n;
        return kRoutine[routine].side ? dm * dn * (side == HIPBLAS_SIDE_RIGHT ? dn : dm) : dn * (dn + 1.0) * (double)k;
    }
};

struct HookStats {
    std::atomic<unsigned long long> emu_calls{0}, nat_calls{0};
    std::atomic<unsigned long long> emu_mflops{0}, nat_mflops{0};  // 2 m n k batch / 1e6 (x 4 for complex), rounded down
    std::atomic<unsigned long long> level3[kRoutines][2][2] = {};  // [routine][emulated, native][calls, mflops (RoutineInfo::stats_flops)]
    static void dump();
    HookStats() { std::atexit(&HookStats::dump); }
};
HookStats& hook_stats() {
    static HookStats* st = new HookStats;  // leaked on purpose: dumped from atexit
    return *st;
}
void HookStats::dump() {
    if (!env_one("GEMMUL8_HOOK_STATS")) return;
    HookStats& h = hook_stats();
    std::fprintf(stderr, "[GEMMUL8 HOOK] stats: emulated %llu GEMM calls (%.3f TFLOP), native %llu GEMM calls through the hooked entry points (%.3f TFLOP)\n",
                 h.emu_calls.load(), h.emu_mflops.load() * 1e-6, h.nat_calls.load(), h.nat_mflops.load() * 1e-6);
    for (int r = 0; r < kRoutines; ++r) {  // a line for each routine that was seen
        const auto& n = h.level3[r];
        if (n[0][0].load() + n[1][0].load())
            std::fprintf(stderr, "[GEMMUL8 HOOK] stats: emulated %llu %s calls (%.3f TFLOP), native %llu %s calls through the hooked entry points (%.3f TFLOP)\n",
                         n[0][0].load(), kRoutine[r].name, n[0][1].load() * 1e-6, n[1][0].load(), kRoutine[r].name, n[1][1].load() * 1e-6);
    }
}
void count_call(bool emulated, const GemmCall& c) {
    static const bool on = env_one("GEMMUL8_HOOK_STATS");
    if (!on) return;
    HookStats& h = hook_stats();
    const unsigned long long mf = (unsigned long long)(2.0 * c.m * c.n * c.k * c.batch * (c.dtype >= 2 ? 4.0 : 1.0) * 1e-6);
    (emulated ? h.emu_calls : h.nat_calls).fetch_add(1, std::memory_order_relaxed);
    (emulated ? h.emu_mflops : h.nat_mflops).fetch_add(mf, std::memory_order_relaxed);
}

struct FloorModel {
    double e[6];  // ms: 1, (m+n)k, N(m+n)k, mn, N mn, N mnk
    double n[3];  // ms: 1, mn, mnk
};
// generated by tools/fit_floor.py from profiles/sweeps/r06_floor_scan_*.csv (the round-6 kernels: accurate mode two launches shorter, short-k epilogue +3-5 %; round 4's fit: r04b_floor_scan_*.csv)
const FloorModel kFloor[4][2] = {  // [S, D, C, Z][accurate, fast]
    {{{0.05373, 2.353e-09, 3.999e-10, 1.821e-09, 3.555e-10, 6.155e-13}, {0.02155, 4.627e-10, 1.407e-11}}, {{0.04309, 1.051e-09, 4.238e-10, 1.091e-09, 3.574e-10, 5.79e-13}, {0.02155, 4.627e-10, 1.407e-11}}},
    {{{0.04743, 3.922e-09, 4.089e-10, 1.218e-09, 5.024e-10, 5.943e-13}, {0.01043, 8.077e-10, 2.819e-11}}, {{0.03986, 1.88e-09, 4.137e-10, 4.544e-10, 4.8e-10, 5.863e-13}, {0.01043, 8.077e-10, 2.819e-11}}},
    {{{0.06931, 6.912e-09, 1.196e-09, 3.604e-09, 1.806e-09, 1.761e-12}, {0.01406, 2.65e-10, 5.735e-11}}, {{0.05653, 2.963e-09, 1.234e-09, 2.005e-09, 1.787e-09, 1.72e-12}, {0.01406, 2.65e-10, 5.735e-11}}},
    {{{0.07734, 1.242e-08, 1.326e-09, 1.842e-09, 2.131e-09, 1.734e-12}, {0.01304, 2.591e-10, 1.098e-10}}, {{0.06313, 7.525e-09, 1.292e-09, 9.713e-10, 2.174e-09, 1.625e-12}, {0.01304, 2.591e-10, 1.098e-10}}},
};
bool floor_model_declines(int dtype, double m, double n, double k, unsigned N, bool fast, int backend, double batch) {
    const FloorModel& fm = kFloor[dtype][fast ? 1 : 0];
    const double mk = (m + n) * k, mn = m * n, mnk = mn * k, Nd = (double)N;
    double te = fm.e[0] + batch * ((fm.e[1] + fm.e[2] * Nd) * mk + (fm.e[3] + fm.e[4] * Nd) * mn + fm.e[5] * Nd * mnk);
    static const double kFp8Factor[4] = {1.75, 1.9, 2.05, 2.1};  // [S, D, C, Z]
    if (backend == GEMMUL8_FP8) te *= kFp8Factor[dtype];
    const double tn = fm.n[0] + batch * (fm.n[1] * mn + fm.n[2] * mnk);
    return te > 0.95 * tn;
}
// quiet = a query (gemmul8_hook_would_emulate), not a call: no log line
bool below_floor(int dtype, double m, double n, double k, unsigned N, bool fast, int backend, double batch = 1.0, bool quiet = false) {
    const char* s = std::getenv("GEMMUL8_MIN_FLOPS");
    if (!s || !*s) return false;  // the reference's behaviour: every selected call is emulated
    bool declined;
    if (s[0] == 'a' || s[0] == 'A') {
        declined = floor_model_declines(dtype, m, n, k, N, fast, backend, batch);
    } else {
        const unsigned long long f = env_u64("GEMMUL8_MIN_FLOPS", 0);
        declined = f && 2.0 * m * n * k < (double)f;
    }
    if (declined && !quiet) {
        static std::once_flag told;
        std::call_once(told, [&] {
            std::fprintf(stderr, "[GEMMUL8 HOOK] GEMMUL8_MIN_FLOPS=%s: a %cGEMM %.0f x %.0f x %.0f (batch %.0f, %u moduli%s) stays on the native routine -- "
                                 "calls below the floor are NOT emulated (this message is printed once)\n",
                         s, "SDCZ"[dtype], m, n, k, batch, N, backend == GEMMUL8_FP8 ? ", FP8 backend: cost x 1.75-2.1" : "");
        });
    }
    return declined;
}
// the same for a Level-3 call on the INT8 backend (RoutineInfo::floor_flops, auto_min_order); the first call of each routine that is declined is logged
bool level3_below_floor(const Level3Call& c, unsigned N, bool fast) {
    const char* s = std::getenv("GEMMUL8_MIN_FLOPS");
    if (!s || !*s) return false;
    const RoutineInfo& ri = kRoutine[c.routine];
    const double m = (double)c.m, n = (double)c.n, k = (double)c.k, ka = c.side == HIPBLAS_SIDE_RIGHT ? n : m;
    bool declined;
    if (s[0] == 'a' || s[0] == 'A') {
        declined = ri.auto_min_order ? ka < (double)ri.auto_min_order
                   : ri.side         ? floor_model_declines(c.dtype, m, n, ka, N, fast, GEMMUL8_INT8, 1.0)
                                     : floor_model_declines(c.dtype, n, n, ri.k_fold * k, N, fast, GEMMUL8_INT8, 1.0);
    } else {
        const unsigned long long f = env_u64("GEMMUL8_MIN_FLOPS", 0);
        declined = f && ri.floor_flops * c.flops() < (double)f;
    }
    if (declined) {
        static std::once_flag told[kRoutines];
        std::call_once(told[c.routine], [&] {
            if (ri.side)
                std::fprintf(stderr, "[GEMMUL8 HOOK] GEMMUL8_MIN_FLOPS=%s: a %c%s m = %.0f, n = %.0f, order of A = %.0f (%u moduli) stays on the native routine -- calls "
                                     "below the floor are NOT emulated (this message is printed once)\n", s, "SDCZ"[c.dtype], ri.name, m, n, ka, N);
            else
                std::fprintf(stderr, "[GEMMUL8 HOOK] GEMMUL8_MIN_FLOPS=%s: a %c%s n = %.0f, k = %.0f (%u moduli) stays on the native routine -- calls below the "
                                     "floor are NOT emulated%s (this message is printed once)\n", s, "SDCZ"[c.dtype], ri.name, n, k, N,
                             c.routine == kHER2K ? "; no HER2K scan has been fitted: a number is a floor on 8 n (n + 1) k, `auto` is the GEMM model's decision for (n, n, k)" : "");
        });
    }
    return declined;
}

// "Does the environment select emulation for this call?": a moduli count in the type's range, and the call not below the floor.  The k
// range is a separate question (k_in_range): the single-call path leaves it to gemmul8_gemm, whose decline is logged once; the batched
// and hipblasLt paths ask first, because they commit to a path (or touch D) before the emulator is called.
bool selected(const GemmCall& c, Selection* s, bool fp8_notice = false) {
    if (!selection_from_env(c.dtype, s)) return false;
    if (fp8_notice && s->backend == GEMMUL8_FP8) {
        // the FP8 backend exists for parity with the reference; on this chip the INT8 backend dominates it: three GEMMs per modulus (on FP6 codes
        // of the backend's integer pieces, 1.5x the INT8 kernel's rate since round 5) against one INT8 GEMM (profiles/sweeps/r05_types_backends.csv:
        // SGEMM 8192^3 193 vs 302 TFLOPS, native 153; DGEMM 101 vs 160, native 71).  Say so once.
        static std::once_flag told;
        std::call_once(told, [] {
            std::fprintf(stderr, "[GEMMUL8 HOOK] GEMMUL8_BACKEND=FP8: on MI355X the INT8 backend (GEMMUL8_BACKEND=0) is 1.6-2x faster at equal or better "
                                 "accuracy for S/D/C/Z; continuing with FP8 as requested\n");
        });
    }
    return !below_floor(c.dtype, c.m, c.n, c.k, s->N, s->fast, s->backend, (double)c.batch);
}

// one GEMM (c.batch == 1) on the handle's stream and buffers; returns true and sets *status when the call was served here (emulated, or
// failed), false -> the caller passes it through
bool try_emulate_impl(hipblasHandle_t handle, const GemmCall& c, hipblasStatus_t* status, const hipStream_t* explicit_stream) {
    Selection s;
    if (!selected(c, &s, true)) return false;
    const int dtype = c.dtype, backend = s.backend;
    const unsigned N = s.N;
    const bool fastmode = s.fast, enA = s.enA, enB = s.enB;

    LockedState l = lock_ordered(handle, explicit_stream);
    if (l.st != HIPBLAS_STATUS_SUCCESS) return *status = l.st, true;
    HandleState* const sp = l.sp.get();
    hipStream_t stream = l.stream;
    hipblasStatus_t st;

    const int dist_kind = dist_kind_from_env();
    if (dist_kind >= 0 && try_dist(dist_kind, c, s, stream, status)) return true;

    size_t needA = 0, needB = 0;
    const size_t tot = abi().work_size(kTypes[dtype].cplx, backend, (size_t)c.m, (size_t)c.n, (size_t)c.k, N, enA, enB, &needA, &needB);
    if (tot < needA + needB) return *status = HIPBLAS_STATUS_INVALID_VALUE, true;
    size_t reqA = needA, reqB = needB, reqC = tot - needA - needB;
    if (enA || enB) {  // keep buffers (hence cached planes) stable across differently sized calls
        if (enA) reqA = std::max(reqA, g_maxA);
        if (enB) reqB = std::max(reqB, g_maxB);
        reqC = std::max(reqC, g_maxC);
    }
    if ((st = grow(sp->wA, reqA, stream, "workA")) != HIPBLAS_STATUS_SUCCESS) return *status = st, true;
    if ((st = grow(sp->wB, reqB, stream, "workB")) != HIPBLAS_STATUS_SUCCESS) return *status = st, true;
    if ((st = grow(sp->wC, reqC, stream, "workC")) != HIPBLAS_STATUS_SUCCESS) return *status = st, true;

    const Cache& o = sp->last;
    bool skipA = false, skipB = false;
    if (o.valid && o.num_moduli == N && o.k == (size_t)c.k && o.dtype == dtype && o.fastmode == fastmode && o.backend == backend && o.enA == enA &&
        o.enB == enB) {
        skipA = enA && o.workA == sp->wA.ptr && o.A == c.A && o.m == (size_t)c.m && o.lda == (size_t)c.lda && o.op_A == (int)c.ta;
        skipB = enB && o.workB == sp->wB.ptr && o.B == c.B && o.n == (size_t)c.n && o.ldb == (size_t)c.ldb && o.op_B == (int)c.tb;
    }
    sp->last.valid = false;  // the call below overwrites the planes; the cache is re-validated only if it succeeds
    const int rc = abi().gemm(stream, dtype, backend, (int)c.ta, (int)c.tb, (size_t)c.m, (size_t)c.n, (size_t)c.k, c.alpha, c.A, (size_t)c.lda, c.B,
                              (size_t)c.ldb, c.beta, c.C, (size_t)c.ldc, N, fastmode, sp->wC.ptr, sp->wA.ptr, sp->wB.ptr, enA, enB, skipA, skipB, nullptr);
    if (rc < 0) {
        // a GEMMUL8_E_* status means "this call is outside what the emulator accepts" (k > 2^17, FP8 with k > 65536, a
        // combination that is not built, ...): nothing has been written to C yet, so the application's call is still valid
        // for the native routine -- pass it through instead of failing a call that works without the hook
        static std::once_flag warned;
        std::call_once(warned, [&] {
            std::fprintf(stderr, "[GEMMUL8 HOOK] emulation declined a call (status %d; type %d, backend %d, m=%d n=%d k=%d): using the native routine for such calls\n",
                         rc, dtype, backend, c.m, c.n, c.k);
        });
        return false;
    }
    if (rc != 0) return *status = HIPBLAS_STATUS_INTERNAL_ERROR, true;  // positive: a hipError_t from the runtime
    Cache& u = sp->last;
    u.valid = true;
    u.enA = enA, u.enB = enB;
    u.num_moduli = N;
    u.op_A = (int)c.ta, u.op_B = (int)c.tb;
    u.m = c.m, u.n = c.n, u.k = c.k, u.lda = c.lda, u.ldb = c.ldb;
    u.A = c.A, u.B = c.B;
    u.workA = sp->wA.ptr, u.workB = sp->wB.ptr;
    u.dtype = dtype, u.backend = backend, u.fastmode = fastmode;
    return *status = HIPBLAS_STATUS_SUCCESS, true;
}
// counted front end (GEMMUL8_HOOK_STATS): true = the call was served here (emulated, or failed with *status set); false = native routine
bool try_emulate(hipblasHandle_t handle, const GemmCall& c, hipblasStatus_t* status, const hipStream_t* explicit_stream = nullptr) {
    if (tl_native_depth > 0) return false;  // inside a native pass-through of an outer hooked entry: the same call, already declined and counted
    const bool served = try_emulate_impl(handle, c, status, explicit_stream);
    count_call(served, c);
    return served;
}

// ---- the gate of the Level-3 routines (kRoutine).  Selection: the type's GEMMUL8_NUM_MOD_* / GEMMUL8_FASTMODE_*, GEMMUL8_BACKEND.  The native routine takes: a
// library without the entry point, a side / fill mode / operation / diag outside what the routine takes (RoutineInfo::ops; an enum value hipBLAS does not
// define included), a moduli count outside the type's range, the FP8 backend, a k (rank-k) or an order of A (side) above RoutineInfo::limit,
// GEMMUL8_NONFINITE=ieee -- the gemmul8_* entry points ignore the non-finite mode, a NaN or Inf operand would come back as finite numbers -- (each said once
// per routine) and a call below GEMMUL8_MIN_FLOPS (level3_below_floor).  GEMMUL8_DIST and the skip-scaling switches do not apply.  The workspace -- that of
// the GEMM the call amounts to (SYR2K: inner dimension 2 pad256(k)), gemmul8_trsm_work_size for TRSM -- grows through wC.
// Returns true and sets *status when the call was served here (emulated, or failed), false -> the caller passes it through.  c has passed try_level3's screens.
bool emulate_level3(hipblasHandle_t handle, const Level3Call& c, hipblasStatus_t* status) {
    const RoutineInfo& ri = kRoutine[c.routine];
    const Abi& abi_ = abi();
    bool present = false;  // a library linked with this file may lack the entry point (OZ2_ABI)
    switch (c.routine) {
    case kSYRK: present = abi_.syrk; break;
    case kHERK: present = abi_.herk; break;
    case kSYR2K: present = abi_.syr2k; break;
    case kHER2K: present = abi_.her2k; break;
    case kSYMM: present = abi_.symm; break;
    case kHEMM: present = abi_.hemm; break;
    case kTRMM: present = abi_.trmm; break;
    case kTRSM: present = abi_.trsm && abi_.trsm_work_size; break;
    case kRoutines: break;
    }
    if (!present) return false;
    if (c.uplo != HIPBLAS_FILL_MODE_UPPER && c.uplo != HIPBLAS_FILL_MODE_LOWER) return false;
    if (ri.side && c.side != HIPBLAS_SIDE_LEFT && c.side != HIPBLAS_SIDE_RIGHT) return false;
    const bool n_ = c.trans == HIPBLAS_OP_N, t_ = c.trans == HIPBLAS_OP_T, c_ = c.trans == HIPBLAS_OP_C;
    switch (ri.ops) {
    case kOpsNT: if (!n_ && !t_) return false; break;
    case kOpsNC: if (!n_ && !c_) return false; break;
    case kOpsNTC: if ((!n_ && !t_ && !c_) || (c.diag != HIPBLAS_DIAG_NON_UNIT && c.diag != HIPBLAS_DIAG_UNIT)) return false; break;
    case kOpsNone: break;
    }
    const int dtype = c.dtype, m = (int)c.m, n = (int)c.n, k = (int)c.k, ka = c.side == HIPBLAS_SIDE_RIGHT ? n : m;
    const int limited = ri.side ? ka : k;  // the dimension the limit is on
    Selection s;
    if (!selection_from_env(dtype, &s)) {
        if (s.N != 0) {
            static std::once_flag told[kRoutines];
            std::call_once(told[c.routine], [&] {
                std::fprintf(stderr, "[GEMMUL8 HOOK] %s=%u is outside 2..%u: %c%s calls use the native routine\n", kTypes[dtype].nmod, s.N,
                             kTypes[dtype].max_moduli, "SDCZ"[dtype], ri.name);
            });
        }
        return false;
    }
    if (s.backend == GEMMUL8_FP8 || limited > ri.limit) {
        static std::once_flag told[kRoutines][2];  // the backend, the size: one notice each
        std::call_once(told[c.routine][s.backend == GEMMUL8_FP8 ? 0 : 1], [&] {
            if (ri.side)
                std::fprintf(stderr, "[GEMMUL8 HOOK] %s is emulated on the INT8 backend for an A of order <= %d only (GEMMUL8_BACKEND=%d, order %d): using the native "
                                     "routine for such calls\n", ri.name, ri.limit, s.backend, ka);
            else
                std::fprintf(stderr, "[GEMMUL8 HOOK] %s is emulated on the INT8 backend for k <= %d only (GEMMUL8_BACKEND=%d, k=%d): using the native routine "
                                     "for such calls\n", ri.name, ri.limit, s.backend, k);
        });
        return false;
    }
    if (nonfinite_ieee()) {
        static std::once_flag told[kRoutines];
        std::call_once(told[c.routine], [&] {
            std::fprintf(stderr, "[GEMMUL8 HOOK] GEMMUL8_NONFINITE=ieee: %s has no NaN / Inf propagation mode and is NOT emulated: using the native routine "
                                 "for such calls\n", ri.name);
        });
        return false;
    }
    if (level3_below_floor(c, s.N, s.fast)) return false;
    LockedState l = lock_ordered(handle, nullptr);
    if (l.st != HIPBLAS_STATUS_SUCCESS) return *status = l.st, true;
    const bool cplx = kTypes[dtype].cplx;
    const size_t sm = (size_t)m, sn = (size_t)n, sk = (size_t)k, lda = (size_t)c.lda, ldb = (size_t)c.ldb, ldc = (size_t)c.ldc;
    const size_t need = c.routine == kTRSM ? abi_.trsm_work_size(cplx, GEMMUL8_INT8, c.side, sm, sn, s.N)
                        : ri.side          ? abi_.work_size(cplx, GEMMUL8_INT8, sm, sn, (size_t)ka, s.N, 0, 0, nullptr, nullptr)
                                           : abi_.work_size(cplx, GEMMUL8_INT8, sn, sn, ri.k_fold == 1 ? sk : ri.k_fold * ((sk + 255) / 256 * 256), s.N, 0, 0, nullptr, nullptr);
    if (const hipblasStatus_t st = grow(l.sp->wC, std::max(need, g_maxC), l.stream, ri.tag); st != HIPBLAS_STATUS_SUCCESS) return *status = st, true;
    void* const work = l.sp->wC.ptr;
    int rc = GEMMUL8_E_ARG;
    switch (c.routine) {
    case kSYRK:
    case kHERK:
        rc = (c.routine == kHERK ? abi_.herk : abi_.syrk)(l.stream, dtype, GEMMUL8_INT8, c.uplo, c.trans, sn, sk, c.alpha, c.A, lda, c.beta, c.C, ldc, s.N, s.fast, work, nullptr);
        break;
    case kSYR2K:
    case kHER2K:
        rc = (c.routine == kHER2K ? abi_.her2k : abi_.syr2k)(l.stream, dtype, GEMMUL8_INT8, c.uplo, c.trans, sn, sk, c.alpha, c.A, lda, c.B, ldb, c.beta, c.C, ldc, s.N, s.fast,
                                                             work, nullptr);
        break;
    case kSYMM:
    case kHEMM:
        rc = (c.routine == kHEMM ? abi_.hemm : abi_.symm)(l.stream, dtype, GEMMUL8_INT8, c.side, c.uplo, sm, sn, c.alpha, c.A, lda, c.B, ldb, c.beta, c.C, ldc, s.N, s.fast, work,
                                                          nullptr);
        break;
    case kTRMM:
        rc = abi_.trmm(l.stream, dtype, GEMMUL8_INT8, c.side, c.uplo, c.trans, c.diag, sm, sn, c.alpha, c.A, lda, c.B, ldb, c.C, ldc, s.N, s.fast, work, nullptr);
        break;
    case kTRSM:
        rc = abi_.trsm(l.stream, dtype, GEMMUL8_INT8, c.side, c.uplo, c.trans, c.diag, sm, sn, c.alpha, c.A, lda, c.C, ldc, s.N, s.fast, work, nullptr);
        break;
    case kRoutines: break;
    }
    if (rc < 0) {  // declined before anything was written: the native routine takes the call (see try_emulate_impl)
        static std::once_flag warned[kRoutines];
        std::call_once(warned[c.routine], [&] {
            if (ri.side)
                std::fprintf(stderr, "[GEMMUL8 HOOK] emulation declined a %s call (status %d; type %d, m=%d n=%d): using the native routine for such calls\n", ri.name, rc,
                             dtype, m, n);
            else
                std::fprintf(stderr, "[GEMMUL8 HOOK] emulation declined a %s call (status %d; type %d, n=%d k=%d): using the native routine for such calls\n", ri.name, rc,
                             dtype, n, k);
        });
        return false;
    }
    return *status = rc == 0 ? HIPBLAS_STATUS_SUCCESS : HIPBLAS_STATUS_INTERNAL_ERROR, true;
}
// counted front end (GEMMUL8_HOOK_STATS); false = the native routine takes the call: also, uncounted, a call inside a native pass-through, an empty call, a null
// pointer (the native routine reports it) and a dimension an int cannot hold
bool try_level3(hipblasHandle_t handle, const Level3Call& c, hipblasStatus_t* status) {
    if (tl_native_depth > 0) return false;
    const RoutineInfo& ri = kRoutine[c.routine];
    const int64_t lim = 2147483647, other = ri.side ? c.m : c.k;
    if (c.n <= 0 || other <= 0 || !c.alpha || !c.A || !c.C || (ri.beta && !c.beta) || (ri.B && !c.B)) return false;
    if (c.n > lim || other > lim || c.lda > lim || c.ldb > lim || c.ldc > lim) return false;
    const bool served = emulate_level3(handle, c, status);
    static const bool on = env_one("GEMMUL8_HOOK_STATS");
    if (on) {
        auto& n = hook_stats().level3[c.routine][served ? 0 : 1];
        n[0].fetch_add(1, std::memory_order_relaxed);
        n[1].fetch_add((unsigned long long)(ri.stats_flops * c.flops() * (c.dtype >= 2 ? 4.0 : 1.0) * 1e-6), std::memory_order_relaxed);
    }
    return served;
}

// lt: the key is a hipblasLtHandle_t (hipblasLtDestroy) -- hipblasGetStream on such an object would be a type confusion
void release_state(hipblasHandle_t handle, bool lt = false) {
    std::shared_ptr<HandleState> sp;
    {
        std::lock_guard<std::mutex> g(g_map_mtx);
        auto it = g_map.find(handle);
        if (it == g_map.end()) return;
        sp = it->second;
        g_map.erase(it);
    }
    std::lock_guard<std::mutex> lk(sp->mtx);
    hipStream_t stream = nullptr;
    bool have = sp->have_stream;
    if (have) stream = sp->last_stream;
    else if (!lt && !sp->is_lt) {
        hipblasStatus_t st;
        stream = handle_stream(handle, &st);
        have = (st == HIPBLAS_STATUS_SUCCESS);
    }
    if (!have) (void)hipDeviceSynchronize();
    for (Buffer* b : {&sp->wA, &sp->wB, &sp->wC}) {
        if (!b->ptr) continue;
        hipError_t e = have ? hipFreeAsync(b->ptr, stream) : hipFree(b->ptr);
        if (e != hipSuccess && have && hipStreamSynchronize(stream) == hipSuccess) e = hipFree(b->ptr);
        if (e != hipSuccess) std::fprintf(stderr, "[GEMMUL8 HOOK] hipblasDestroy: freeing a workspace failed (%s)\n", hipGetErrorString(e));
        b->ptr = nullptr;
        b->size = 0;
    }
    if (sp->last_event) (void)hipEventDestroy(sp->last_event), sp->last_event = nullptr;
    for (BatchLane& ln : sp->lanes) {
        if (ln.w.ptr) {
            hipError_t e = ln.stream ? hipFreeAsync(ln.w.ptr, ln.stream) : hipFree(ln.w.ptr);
            if (e == hipSuccess && ln.stream) e = hipStreamSynchronize(ln.stream);
            if (e != hipSuccess) std::fprintf(stderr, "[GEMMUL8 HOOK] hipblasDestroy: freeing a batch workspace failed (%s)\n", hipGetErrorString(e));
            ln.w = Buffer{};
        }
        if (ln.done) (void)hipEventDestroy(ln.done), ln.done = nullptr;
        if (ln.stream) (void)hipStreamDestroy(ln.stream), ln.stream = nullptr;
    }
    if (sp->fork) (void)hipEventDestroy(sp->fork), sp->fork = nullptr;
}

// Strided-batched entry points (not hooked by the reference; PyTorch's bmm uses them).  alpha/beta are shared by the batch; element
// strides are in units of the matrix type.  The items of a batch are independent, and below ~2048^3 one emulated GEMM is ten
// latency-bound launches that leave most of the chip idle.  Default: one set of launches for the whole batch (below).  Otherwise
// (GEMMUL8_BATCH_FUSED=0, GEMMUL8_DIST) the batch is spread over GEMMUL8_BATCH_STREAMS lanes (default 4, 1 =
// serial loop on the handle's stream): lane 0 is the handle's stream with the handle's buffers, every other lane has its own
// non-blocking stream and workspace; the lanes fork from the handle's stream with an event and join it again before the call
// returns, so the call stays stream-ordered for the application (and capturable in a HIP graph after one warm-up call).
bool emulate_batch(hipblasHandle_t handle, const GemmCall& c, hipblasStatus_t* status, const hipStream_t* explicit_stream = nullptr) {
    *status = HIPBLAS_STATUS_SUCCESS;
    if (tl_native_depth > 0) return false;  // see try_emulate
    const int dtype = c.dtype, batch = c.batch;
    const long long elem = (long long)c.elem;
    Selection s;
    // First choice (GEMMUL8_BATCH_FUSED != 0): the whole batch as ONE set of launches (gemmul8_gemm_batched: the items in
    // gridDim.z of every kernel) -- a batch of small matrices then fills the chip and costs ten launches, not ten per item.
    if (batch > 1 && env_u64("GEMMUL8_BATCH_FUSED", 1) != 0 && dist_kind_from_env() < 0) {
        if (!selected(c, &s)) return false;
        if (k_in_range(c, s)) {
            LockedState l = lock_ordered(handle, explicit_stream);
            if (l.st != HIPBLAS_STATUS_SUCCESS) return *status = l.st, true;
            HandleState* const sp = l.sp.get();
            hipStream_t stream = l.stream;
            // the items' workspaces are consecutive: bound the buffer (GEMMUL8_BATCH_WORKSPACE_MB, default 4096) and run the batch in
            // chunks of as many items as fit; if even that cannot be allocated the per-item path below takes over
            const size_t item = abi().work_size_batched(kTypes[dtype].cplx, s.backend, (size_t)c.m, (size_t)c.n, (size_t)c.k, s.N, 1) - 256;
            const size_t budget = (size_t)env_u64("GEMMUL8_BATCH_WORKSPACE_MB", 4096) << 20;
            const size_t per_chunk = std::max<size_t>(1, std::min<size_t>((size_t)batch, item ? budget / item : (size_t)batch));
            if (grow(sp->wC, item * per_chunk + 256, stream, "workC (batched)") == HIPBLAS_STATUS_SUCCESS) {
                sp->last.valid = false;  // the skip-scaling cache describes single calls; the planes are overwritten here
                int rc = 0;
                for (size_t b0 = 0; b0 < (size_t)batch && rc == 0; b0 += per_chunk) {
                    const size_t nb = std::min(per_chunk, (size_t)batch - b0);
                    rc = abi().gemm_batched(stream, dtype, s.backend, (int)c.ta, (int)c.tb, (size_t)c.m, (size_t)c.n, (size_t)c.k, c.alpha,
                                            (const char*)c.A + (long long)b0 * c.sa * elem, (size_t)c.lda, c.sa,
                                            (const char*)c.B + (long long)b0 * c.sb * elem, (size_t)c.ldb, c.sb, c.beta,
                                            (char*)c.C + (long long)b0 * c.sc * elem, (size_t)c.ldc, c.sc, nb, s.N, s.fast, sp->wC.ptr);
                    if (rc < 0 && b0 > 0) rc = 1;  // declined after earlier chunks were written: cannot hand the call to another path
                }
                if (rc == 0) return count_call(true, c), true;
                if (rc > 0) return *status = HIPBLAS_STATUS_INTERNAL_ERROR, true;
                // negative on the first chunk: declined (nothing written) -- fall through to the per-item path
            } else {
                (void)hipGetLastError();  // allocation failed: clear the sticky error, use the per-item path
            }
        }
    }
    auto item = [&](int b) {
        GemmCall it = c;
        it.A = (const char*)c.A + (size_t)b * c.sa * c.elem, it.B = (const char*)c.B + (size_t)b * c.sb * c.elem, it.C = (char*)c.C + (size_t)b * c.sc * c.elem;
        it.batch = 1;
        return it;
    };
    hipblasStatus_t st;
    // item 0 on the handle's stream decides whether the environment selects emulation for this call at all
    if (!try_emulate(handle, item(0), &st, explicit_stream)) return false;
    if (st != HIPBLAS_STATUS_SUCCESS) return *status = st, true;
    int lanes = (int)env_u64("GEMMUL8_BATCH_STREAMS", 4);
    lanes = std::max(1, std::min({lanes, kMaxBatchLanes, batch}));
    (void)selection_from_env(dtype, &s);  // item 0 was served with it
    if (lanes > 1 && dist_kind_from_env() >= 0) lanes = 1;  // the sharded path keeps its collectives on one stream
    auto sp = state_of(handle);
    hipStream_t main_stream = nullptr;
    if (lanes > 1) {
        std::lock_guard<std::mutex> lk(sp->mtx);
        main_stream = sp->last_stream;  // set by item 0
        bool ok = sp->fork || hipEventCreateWithFlags(&sp->fork, hipEventDisableTiming) == hipSuccess;
        const size_t need = abi().work_size(kTypes[dtype].cplx, s.backend, (size_t)c.m, (size_t)c.n, (size_t)c.k, s.N, 0, 0, nullptr, nullptr);
        ok = ok && hipEventRecord(sp->fork, main_stream) == hipSuccess;
        for (int l = 1; l < lanes && ok; ++l) {
            BatchLane& ln = sp->lanes[l];
            if (!ln.stream) ok = hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking) == hipSuccess;
            if (ok && !ln.done) ok = hipEventCreateWithFlags(&ln.done, hipEventDisableTiming) == hipSuccess;
            ok = ok && hipStreamWaitEvent(ln.stream, sp->fork, 0) == hipSuccess;
            ok = ok && grow(ln.w, need, ln.stream, "batch lane") == HIPBLAS_STATUS_SUCCESS;
        }
        if (!ok) lanes = 1;  // fall back to the serial loop
    }
    for (int b = 1; b < batch; ++b) {
        const GemmCall it = item(b);
        const int l = b % lanes;
        if (l == 0) {
            const bool done = try_emulate(handle, it, &st, explicit_stream);
            if (!done || st != HIPBLAS_STATUS_SUCCESS) {  // stop issuing items; the forked lanes are still joined below
                *status = done ? st : HIPBLAS_STATUS_INTERNAL_ERROR;
                break;
            }
        } else {
            std::lock_guard<std::mutex> lk(sp->mtx);
            BatchLane& ln = sp->lanes[l];
            const int rc = abi().gemm(ln.stream, dtype, s.backend, (int)c.ta, (int)c.tb, (size_t)c.m, (size_t)c.n, (size_t)c.k, c.alpha, it.A, (size_t)c.lda, it.B,
                                      (size_t)c.ldb, c.beta, it.C, (size_t)c.ldc, s.N, s.fast, ln.w.ptr, nullptr, nullptr, 0, 0, 0, 0, nullptr);
            if (rc != 0) *status = HIPBLAS_STATUS_INTERNAL_ERROR;  // item 0 ran with the same shape and switches: should not happen
        }
    }
    if (lanes > 1) {  // join: the handle's stream waits for every lane
        std::lock_guard<std::mutex> lk(sp->mtx);
        for (int l = 1; l < lanes; ++l) {
            BatchLane& ln = sp->lanes[l];
            if (hipEventRecord(ln.done, ln.stream) != hipSuccess || hipStreamWaitEvent(main_stream, ln.done, 0) != hipSuccess)
                *status = HIPBLAS_STATUS_INTERNAL_ERROR;
        }
    }
    return true;
}

// Pointer-array batches (hipblas?gemmBatched, hipblasGemmBatchedEx, rocblas_?gemm_batched; not hooked by the reference): c.A / c.B / c.C are the three
// DEVICE arrays of item addresses, c.sa / c.sb / c.sc are unused.  The hook never reads an array: the only path is the fused one (gemmul8_gemm_batched_ptr:
// the kernels load their item's entries in stream order; capturable), for every batch >= 1.  The stream-lane and serial forms of emulate_batch walk item
// addresses on the host and do not exist here: what they would take goes to the native routine, said once.  GEMMUL8_BATCH_WORKSPACE_MB chunks the batch as
// for the strided form, by offsetting the three arrays (host arithmetic on the arrays' own addresses).  The `auto` floor is the strided batches' model.
// GEMMUL8_HOOK_STATS: every call that arrives here is counted once, emulated or native, as try_emulate counts single GEMMs.
bool emulate_batch_ptr(hipblasHandle_t handle, const GemmCall& c, hipblasStatus_t* status, const hipStream_t* explicit_stream = nullptr) {
    *status = HIPBLAS_STATUS_SUCCESS;
    if (tl_native_depth > 0) return false;  // see try_emulate
    enum { kNoFused, kDist, kNoSymbol, kNoWorkspace, kModuli, kKRange, kDeclined, kReasons };
    auto native = [&](int why, long long detail = 0) {
        static std::once_flag told[kReasons];
        static const char* const text[kReasons] = {
            "GEMMUL8_BATCH_FUSED=0: only the fused path can serve a pointer-array batch (the arrays are not read on the host)",
            "GEMMUL8_DIST is set: the multi-GPU plans do not take pointer-array batches",
            "the library has no gemmul8_gemm_batched_ptr",
            "the workspace of the first chunk could not be allocated",
            "the moduli count of GEMMUL8_NUM_MOD_{S,D,C,Z} is outside the type's range",
            "k is beyond the emulator's range",
            "the emulator declined the call",
        };
        std::call_once(told[why], [&] {
            char num[32] = "";
            if (detail) std::snprintf(num, sizeof num, " (%lld)", detail);
            std::fprintf(stderr, "[GEMMUL8 HOOK] pointer-array batched %cGEMM %d x %d x %d (batch %d): %s%s -- using the native routine for such calls "
                                 "(this message is printed once)\n", "SDCZ"[c.dtype], c.m, c.n, c.k, c.batch, text[why], num);
        });
        count_call(false, c);
        return false;
    };
    const int dtype = c.dtype;
    Selection s;
    if (!selection_from_env(dtype, &s)) {
        if (s.N != 0) return native(kModuli, (long long)s.N);  // asked for, but not a count the type has
        return count_call(false, c), false;                     // the environment does not ask for this type: silent, as everywhere
    }
    if (!selected(c, &s, true)) return count_call(false, c), false;  // below the floor (logged once by below_floor)
    if (env_u64("GEMMUL8_BATCH_FUSED", 1) == 0) return native(kNoFused);
    if (dist_kind_from_env() >= 0) return native(kDist);
    const auto fn = abi().gemm_batched_ptr;
    if (!fn) return native(kNoSymbol);
    if (!k_in_range(c, s)) return native(kKRange, c.k);
    LockedState l = lock_ordered(handle, explicit_stream);
    if (l.st != HIPBLAS_STATUS_SUCCESS) return *status = l.st, true;
    HandleState* const sp = l.sp.get();
    hipStream_t stream = l.stream;
    const size_t batch = (size_t)c.batch;
    const size_t item = abi().work_size_batched(kTypes[dtype].cplx, s.backend, (size_t)c.m, (size_t)c.n, (size_t)c.k, s.N, 1) - 256;
    const size_t budget = (size_t)env_u64("GEMMUL8_BATCH_WORKSPACE_MB", 4096) << 20;
    const size_t per_chunk = std::max<size_t>(1, std::min<size_t>(batch, item ? budget / item : batch));
    if (grow(sp->wC, item * per_chunk + 256, stream, "workC (pointer-array batch)") != HIPBLAS_STATUS_SUCCESS) {
        (void)hipGetLastError();  // allocation failed: clear the sticky error
        return native(kNoWorkspace, (long long)(item * per_chunk + 256));
    }
    sp->last.valid = false;  // the skip-scaling cache describes single calls; the planes are overwritten here
    const void* const* pa = (const void* const*)c.A;
    const void* const* pb = (const void* const*)c.B;
    void* const* pc = (void* const*)c.C;
    for (size_t b0 = 0; b0 < batch; b0 += per_chunk) {
        const size_t nb = std::min(per_chunk, batch - b0);
        const int rc = fn(stream, dtype, s.backend, (int)c.ta, (int)c.tb, (size_t)c.m, (size_t)c.n, (size_t)c.k, c.alpha, pa + b0, (size_t)c.lda, pb + b0,
                          (size_t)c.ldb, c.beta, pc + b0, (size_t)c.ldc, nb, s.N, s.fast, sp->wC.ptr);
        if (rc < 0 && b0 == 0) return native(kDeclined, rc);  // nothing written yet: the call is still the native routine's
        if (rc != 0) return *status = HIPBLAS_STATUS_INTERNAL_ERROR, true;
    }
    return count_call(true, c), true;
}


// ---- rocBLAS entry points, opt-in with GEMMUL8_HOOK_ROCBLAS=1 (no counterpart in the reference: src/hook.cu:846-1055 hooks the cuBLAS / hipBLAS
// names only).  For applications that call rocBLAS directly.  The handle of a hipBLAS call IS the rocBLAS handle, so a call the hipBLAS hooks
// declined arrives here again through the real hipBLAS and is declined again by the same rules.  rocblas_operation / rocblas_status are plain
// ints here (111 / 112 / 113 = the hipBLAS values; 0 = success, 6 = internal error); rocblas_int is 32-bit in this build of rocBLAS
// (rocblas-types.h:79).
bool rocblas_stream(void* handle, hipStream_t* s) {
    static const auto fn = real<decltype(&rocblas_get_stream)>("rocblas_get_stream");
    return fn && fn(handle, s) == 0;
}
int rocblas_status_of(hipblasStatus_t st) { return st == HIPBLAS_STATUS_SUCCESS ? 0 : st == HIPBLAS_STATUS_ALLOC_FAILED ? 5 : 6; }

// rocblas_internal_gemm_template is an INTERNAL, unversioned C++ symbol: the mangled name pins the parameter TYPES but not their meaning
// (offsets in elements, strides, the batch count), and a ROCm point release may change those without changing the name -- silent argument
// corruption instead of a clean pass-through.  The interposition is therefore limited to the rocBLAS releases it was run against
// (tests/test_gpu_hook_reach.py on PyTorch's bundled 5.0.x, tests/cpp/test_hook_rocblas.cpp on ROCm 7.2's 5.2.x); any other version string
// -- or a rocBLAS without rocblas_get_version_string -- takes the pass-through, with one log line.  GEMMUL8_ROCBLAS_ABI_UNCHECKED=1 overrides.
constexpr const char* kTestedRocblas[] = {"5.0.", "5.2."};
bool rocblas_version_tested(const char* v) {
    if (!v) return false;
    for (const char* pre : kTestedRocblas)
        if (std::strncmp(v, pre, std::strlen(pre)) == 0) return true;
    return false;
}
bool rocblas_internal_abi_ok() {
    static const bool ok = [] {
        if (env_one("GEMMUL8_ROCBLAS_ABI_UNCHECKED")) return true;
        const auto fsz = real<decltype(&rocblas_get_version_string_size)>("rocblas_get_version_string_size");
        const auto fstr = real<decltype(&rocblas_get_version_string)>("rocblas_get_version_string");
        char buf[128] = "";
        size_t len = 0;
        const bool have = fsz && fstr && fsz(&len) == 0 && len > 0 && len <= sizeof(buf) && fstr(buf, len) == 0;
        const bool good = have && rocblas_version_tested(buf);
        if (!good && env_one("GEMMUL8_HOOK_ROCBLAS"))
            std::fprintf(stderr, "[GEMMUL8 HOOK] rocBLAS version '%s' is not one this build was tested with (5.0.x, 5.2.x): rocblas_internal_gemm_template "
                                 "(rocSOLVER's trailing updates) is NOT intercepted; the exported rocblas_*gemm entry points still are "
                                 "(GEMMUL8_ROCBLAS_ABI_UNCHECKED=1 overrides)\n", have ? buf : "unknown");
        return good;
    }();
    return ok;
}
// What every rocBLAS entry point asks once the call itself is one for the emulator (gemm_call): the opt-in switch, for the internal
// template the tested release, operations the emulator knows, and -- last, only after all the cheaper tests -- the handle's stream.
bool rocblas_takes(void* handle, int transA, int transB, hipStream_t* s, bool internal_template = false) {
    return env_one("GEMMUL8_HOOK_ROCBLAS") && (!internal_template || rocblas_internal_abi_ok()) && handle && transA >= 111 && transA <= 113 &&
           transB >= 111 && transB <= 113 && rocblas_stream(handle, s);
}

// rocSOLVER / hipSOLVER factorizations (getrf, geqrf, potrf ...: what torch.linalg.lu_factor / solve / qr run on) do not call rocBLAS's C
// entry points: their trailing updates go through rocBLAS's exported C++ template rocblas_internal_gemm_template<T> (and its _64 form).
// Those ARE dynamic symbols, so the same opt-in interposes them -- by their mangled names, which belong to THIS rocBLAS ABI (ROCm 7.2:
// nm -D librocsolver.so | grep internal_gemm); if a later rocBLAS changes the signature the names no longer match, nothing is intercepted,
// and tests/test_gpu_hook_reach.py says so.  Strided batch (batch_count > 1) and element offsets as rocBLAS defines them.
// real_: the routine behind the mangled name, one per <T, I>, resolved once by the caller.
template <typename T, typename I, typename Fn>
int rocblas_internal_gemm_hook(Fn real_, int code, void* handle, int transA, int transB, I m, I n, I k, const T* alpha, const T* A, long offA, I lda,
                               long strideA, const T* B, long offB, I ldb, long strideB, const T* beta, T* C, long offC, I ldc, long strideC, I batch) {
    GemmCall c;
    hipStream_t s_;
    hipblasStatus_t st_;
    if (gemm_call(&c, code, transA, transB, m, n, k, alpha, A ? A + offA : A, lda, strideA, B ? B + offB : B, ldb, strideB, beta, C ? C + offC : C, ldc,
                  strideC, batch) &&
        alpha && beta && rocblas_takes(handle, transA, transB, &s_, true) &&
        (c.batch == 1 ? try_emulate(handle, c, &st_, &s_) : emulate_batch(handle, c, &st_, &s_)))
        return rocblas_status_of(st_);
    NativeScope ns_;
    return real_ ? real_(handle, transA, transB, m, n, k, alpha, A, offA, lda, strideA, B, offB, ldb, strideB, beta, C, offC, ldc, strideC, batch) : 6;
}

// ---- hipblasLtMatmul (not hooked by the reference; PyTorch on ROCm routes most float32 matmuls through hipBLASLt, so without
// this GEMMUL8_NUM_MOD_S is a no-op for them).  Only the plain case is emulated: D = alpha*op(A)*op(B) + beta*C with A, B, C, D of
// one type in {float, double, complex float, complex double}, column-major order, single or strided-batched, default epilogue, no scale pointers,
// host or device scalars; everything else goes to the real routine untouched.  C != D is served in place on D after a copy of C.
struct LtLayout {
    int32_t type = -1, order = -1, batch = 1;
    uint64_t rows = 0, cols = 0;
    int64_t ld = 0;
    int64_t stride = 0;  // STRIDED_BATCH_OFFSET, elements
};
// hipBLASLt (ROCm 7.2) cannot be asked what a matrix layout holds -- hipblasLtMatrixLayoutGetAttribute answers only the two batch
// attributes -- so the hook records type / rows / cols / ld / order / batch when a layout is created or modified
// (hipblasLtMatrixLayoutCreate / SetAttribute / Destroy are interposed below) and reads its own table here.
std::mutex g_lt_mtx;
std::unordered_map<hipblasLtMatrixLayout_t, LtLayout> g_lt_layouts;
bool lt_layout(hipblasLtMatrixLayout_t L, LtLayout* o) {
    std::lock_guard<std::mutex> g(g_lt_mtx);
    auto it = g_lt_layouts.find(L);
    if (it == g_lt_layouts.end()) return false;  // created before the hook was loaded, or by an interface we do not see
    *o = it->second;
    return true;
}
// GEMMUL8_HOOK_VERBOSE=1: say why a hipblasLtMatmul call was left to the native routine
bool lt_decline(const char* why) {
    if (env_one("GEMMUL8_HOOK_VERBOSE")) std::fprintf(stderr, "[GEMMUL8 HOOK] hipblasLtMatmul -> native: %s\n", why);
    return false;
}
// returns true when the call was emulated (status in *st)
bool lt_try(hipblasLtHandle_t handle, hipblasLtMatmulDesc_t desc, const void* alpha, const void* A, hipblasLtMatrixLayout_t Ad, const void* B,
            hipblasLtMatrixLayout_t Bd, const void* beta, const void* C, hipblasLtMatrixLayout_t Cd, void* D, hipblasLtMatrixLayout_t Dd,
            hipStream_t stream, hipblasStatus_t* st) {
    if (!desc || !alpha || !beta || !A || !B || !D) return lt_decline("null argument");
    static const auto dget = real<decltype(&hipblasLtMatmulDescGetAttribute)>("hipblasLtMatmulDescGetAttribute");
    if (!dget) return lt_decline("hipblasLtMatmulDescGetAttribute not found");
    size_t w = 0;
    int32_t ta = 0, tb = 0;
    uint32_t epi = 0;
    if (dget(desc, HIPBLASLT_MATMUL_DESC_TRANSA, &ta, sizeof ta, &w) != HIPBLAS_STATUS_SUCCESS) return lt_decline("TRANSA unreadable");
    if (dget(desc, HIPBLASLT_MATMUL_DESC_TRANSB, &tb, sizeof tb, &w) != HIPBLAS_STATUS_SUCCESS) return lt_decline("TRANSB unreadable");
    if (dget(desc, HIPBLASLT_MATMUL_DESC_EPILOGUE, &epi, sizeof epi, &w) != HIPBLAS_STATUS_SUCCESS ||
        (epi != HIPBLASLT_EPILOGUE_DEFAULT && epi != HIPBLASLT_EPILOGUE_BIAS))
        return lt_decline("epilogue is neither the default one nor a plain bias");
    // BIAS epilogue (what a float32 torch.nn.Linear issues): D = alpha*op(A)*op(B) + beta*C + bias, bias broadcast over the columns --
    // emulated as the plain GEMM followed by the bias addition when the bias vector has the matrices' (real) type
    const void* bias = nullptr;
    if (epi == HIPBLASLT_EPILOGUE_BIAS) {
        if (dget(desc, HIPBLASLT_MATMUL_DESC_BIAS_POINTER, &bias, sizeof bias, &w) != HIPBLAS_STATUS_SUCCESS || !bias) return lt_decline("bias epilogue without a bias pointer");
    }
    for (auto attr : {HIPBLASLT_MATMUL_DESC_A_SCALE_POINTER, HIPBLASLT_MATMUL_DESC_B_SCALE_POINTER, HIPBLASLT_MATMUL_DESC_C_SCALE_POINTER,
                      HIPBLASLT_MATMUL_DESC_D_SCALE_POINTER, HIPBLASLT_MATMUL_DESC_AMAX_D_POINTER}) {
        void* ptr = nullptr;
        if (dget(desc, attr, &ptr, sizeof ptr, &w) == HIPBLAS_STATUS_SUCCESS && ptr) return lt_decline("scale / amax pointer set");
    }
    int32_t pmode = 0;
    if (dget(desc, HIPBLASLT_MATMUL_DESC_POINTER_MODE, &pmode, sizeof pmode, &w) == HIPBLAS_STATUS_SUCCESS && pmode != HIPBLASLT_POINTER_MODE_HOST &&
        pmode != HIPBLASLT_POINTER_MODE_DEVICE)
        return lt_decline("device-vector scalars");
    LtLayout a, b, c, d;
    if (!lt_layout(Ad, &a) || !lt_layout(Bd, &b) || !lt_layout(Dd, &d)) return lt_decline("a matrix layout was not created under the hook");
    const bool haveC = C && Cd;
    if (haveC && !lt_layout(Cd, &c)) return lt_decline("the C layout was not created under the hook");
    if (!haveC) c = d;
    if (a.type != b.type || a.type != d.type || c.type != d.type) return lt_decline("mixed matrix types");
    const int dtype = dtype_of(a.type);
    if (dtype < 0) return lt_decline("not an S/D/C/Z matrix type");
    if (bias) {
        int32_t bt = a.type;
        // an unset BIAS_DATA_TYPE reads back as 255 (invalid) in ROCm 7.2 and means "the type of D"
        if (dget(desc, HIPBLASLT_MATMUL_DESC_BIAS_DATA_TYPE, &bt, sizeof bt, &w) != HIPBLAS_STATUS_SUCCESS || (bt != a.type && bt != 255))
            return lt_decline("bias vector of another type than the matrices");
        if (dtype != GEMMUL8_S && dtype != GEMMUL8_D) return lt_decline("bias epilogue on a complex type");
        if (d.batch != 1 || d.cols > 65535) return lt_decline("bias epilogue on a batched or very wide product");
    }
    if (a.order != HIPBLASLT_ORDER_COL || b.order != HIPBLASLT_ORDER_COL || c.order != HIPBLASLT_ORDER_COL || d.order != HIPBLASLT_ORDER_COL) return lt_decline("not column-major");
    const int nb = d.batch;
    if (nb < 1 || a.batch != nb || b.batch != nb || c.batch != nb) return lt_decline("batch counts differ between the layouts");
    if (nb > 1 && d.stride == 0) return lt_decline("batched with overlapping outputs");
    const uint64_t m = d.rows, n = d.cols, k = (ta == HIPBLAS_OP_N) ? a.cols : a.rows;
    if ((ta == HIPBLAS_OP_N ? a.rows : a.cols) != m || (tb == HIPBLAS_OP_N ? b.cols : b.rows) != n || (tb == HIPBLAS_OP_N ? b.rows : b.cols) != k)
        return lt_decline("inconsistent dimensions");
    if (c.rows != m || c.cols != n || m == 0 || n == 0 || k == 0) return lt_decline("C / D shape");
    GemmCall g;
    if (!gemm_call(&g, dtype, ta, tb, (int64_t)m, (int64_t)n, (int64_t)k, alpha, A, a.ld, a.stride, B, b.ld, b.stride, beta, D, d.ld, d.stride, nb) ||
        c.ld > 2147483647)
        return false;
    const size_t esz = g.elem;
    // cheap env test before touching D: is emulation selected for this call at all, and is it one the emulator takes?
    Selection s;
    if (!selected(g, &s) || !k_in_range(g, s)) return false;
    // C is not read when the host scalar beta is 0 (the CRT's "C = +-AB" forms and its general form with beta == 0, oz2_crt.hip): then
    // the out-of-place form needs no copy of C into D.  Device scalars: beta is unknown here, C is copied (the kernel still skips
    // reading it when *beta == 0).
    bool c_unread = false;
    if (pmode == HIPBLASLT_POINTER_MODE_HOST) {
        const bool single = dtype == GEMMUL8_S || dtype == GEMMUL8_C;
        const double br = single ? ((const float*)beta)[0] : ((const double*)beta)[0];
        const double bi2 = !kTypes[dtype].cplx ? 0 : single ? ((const float*)beta)[1] : ((const double*)beta)[1];
        c_unread = br == 0 && bi2 == 0;
    }
    if (haveC && C != D && !c_unread) {  // out-of-place form: bring C into D, then update D in place
        for (int bi = 0; bi < nb; ++bi)
            if (hipMemcpy2DAsync((char*)D + (long long)bi * d.stride * (long long)esz, (size_t)d.ld * esz,
                                 (const char*)C + (long long)bi * c.stride * (long long)esz, (size_t)c.ld * esz, m * esz, n,
                                 hipMemcpyDeviceToDevice, stream) != hipSuccess)
                return *st = HIPBLAS_STATUS_INTERNAL_ERROR, true;
    }
    if (nb > 1)  // strided batch (torch.bmm in float32 arrives here): one set of launches, as for hipblas*gemmStridedBatched
        return emulate_batch((hipblasHandle_t)handle, g, st, &stream);
    const bool done = try_emulate((hipblasHandle_t)handle, g, st, &stream);
    if (done && bias && *st == HIPBLAS_STATUS_SUCCESS &&
        abi().add_row_bias(stream, dtype, (size_t)m, (size_t)n, D, (size_t)d.ld, bias) != 0)
        *st = HIPBLAS_STATUS_INTERNAL_ERROR;
    return done;
}

// the plain GEMM entry points' contract (hook.cu:616-617): true = answered here, with *st
bool plain_gemm(hipblasHandle_t handle, int dtype, hipblasOperation_t ta, hipblasOperation_t tb, int64_t m, int64_t n, int64_t k, const void* alpha,
                const void* A, int64_t lda, const void* B, int64_t ldb, const void* beta, void* C, int64_t ldc, hipblasStatus_t* st) {
    if (m <= 0 || n <= 0 || k <= 0) return *st = HIPBLAS_STATUS_SUCCESS, true;
    if (!A || !B || !C) return *st = HIPBLAS_STATUS_INVALID_VALUE, true;
    GemmCall c;
    return gemm_call(&c, dtype, ta, tb, m, n, k, alpha, A, lda, 0, B, ldb, 0, beta, C, ldc, 0) && try_emulate(handle, c, st);
}
// Strided-batched entry points (not hooked by the reference; PyTorch's bmm uses them): no early out -- a degenerate or null argument is
// the native routine's to answer.  alpha / beta are shared by the batch; element strides are in units of the matrix type.
bool batched_gemm(hipblasHandle_t handle, int dtype, hipblasOperation_t ta, hipblasOperation_t tb, int m, int n, int k, const void* alpha, const void* A,
                  int lda, long long sa, const void* B, int ldb, long long sb, const void* beta, void* C, int ldc, long long sc, int batch,
                  hipblasStatus_t* st) {
    GemmCall c;
    return gemm_call(&c, dtype, ta, tb, m, n, k, alpha, A, lda, sa, B, ldb, sb, beta, C, ldc, sc, batch) && alpha && beta && emulate_batch(handle, c, st);
}
// Pointer-array entry points: the same contract (no early out).  A, B, C are the device arrays of item addresses; they ride in the call record's
// A / B / C with strides 0 and are only ever handed on (emulate_batch_ptr).
bool batched_ptr_gemm(hipblasHandle_t handle, int dtype, int ta, int tb, int64_t m, int64_t n, int64_t k, const void* alpha, const void* A, int64_t lda,
                      const void* B, int64_t ldb, const void* beta, const void* C, int64_t ldc, int64_t batch, hipblasStatus_t* st,
                      const hipStream_t* explicit_stream = nullptr) {
    GemmCall c;
    return gemm_call(&c, dtype, ta, tb, m, n, k, alpha, A, lda, 0, B, ldb, 0, beta, const_cast<void*>(C), ldc, 0, batch) && alpha && beta &&
           emulate_batch_ptr(handle, c, st, explicit_stream);
}

}  // namespace

// ---- the exported symbols: everything above is local to this file, everything below has default visibility
#pragma GCC visibility push(default)
extern "C" {

int gemmul8_hook_would_emulate(int dtype, int backend, size_t m, size_t n, size_t k, unsigned num_moduli, int fastmode, size_t batch) {
    if (dtype < 0 || dtype > 3 || (backend != GEMMUL8_INT8 && backend != GEMMUL8_FP8) || batch == 0 || num_moduli < 2 ||
        num_moduli > kTypes[dtype].max_moduli)
        return GEMMUL8_E_ARG;
    if (m == 0 || n == 0 || k == 0) return 0;
    return below_floor(dtype, (double)m, (double)n, (double)k, num_moduli, fastmode != 0, backend, (double)batch, true) ? 0 : 1;
}
int gemmul8_hook_rocblas_version_tested(const char* version) { return rocblas_version_tested(version) ? 1 : 0; }

hipblasStatus_t hipblasDestroy(hipblasHandle_t handle) {
    release_state(handle);
    OZ2_NATIVE(hipblasDestroy, HIPBLAS_STATUS_NOT_INITIALIZED, handle);
}

// I = int, or int64_t for the ILP64 twins of ROCm 7: the same emulation when every dimension fits an int, the native routine otherwise
#define OZ2_GEMM_HOOK(NAME, T, I, CODE)                                                                                                 \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasOperation_t transA, hipblasOperation_t transB, I m, I n, I k, const T* alpha,   \
                         const T* A, I lda, const T* B, I ldb, const T* beta, T* C, I ldc) {                                            \
        hipblasStatus_t st;                                                                                                             \
        if (plain_gemm(handle, CODE, transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, &st)) return st;                     \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc);         \
    }
#define OZ2_SB_HOOK(NAME, T, CODE)                                                                                                      \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasOperation_t transA, hipblasOperation_t transB, int m, int n, int k,              \
                         const T* alpha, const T* A, int lda, long long strideA, const T* B, int ldb, long long strideB, const T* beta, \
                         T* C, int ldc, long long strideC, int batchCount) {                                                            \
        hipblasStatus_t st;                                                                                                             \
        if (batched_gemm(handle, CODE, transA, transB, m, n, k, alpha, A, lda, strideA, B, ldb, strideB, beta, C, ldc, strideC,         \
                         batchCount, &st))                                                                                              \
            return st;                                                                                                                  \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, transA, transB, m, n, k, alpha, A, lda, strideA, B, ldb, strideB,      \
                   beta, C, ldc, strideC, batchCount);                                                                                  \
    }
#define OZ2_PB_HOOK(NAME, T, I, CODE)                                                                                                   \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasOperation_t transA, hipblasOperation_t transB, I m, I n, I k, const T* alpha,   \
                         const T* const A[], I lda, const T* const B[], I ldb, const T* beta, T* const C[], I ldc, I batchCount) {      \
        hipblasStatus_t st;                                                                                                             \
        if (batched_ptr_gemm(handle, CODE, transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, batchCount, &st)) return st;   \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, batchCount); \
    }
// hipblasGemmBatchedEx and its _64 / WithFlags twins: the type / compute combinations of the strided Ex hook (dtype_of)
#define OZ2_PB_EX_HOOK(NAME, I, ...)                                                                                                    \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasOperation_t transA, hipblasOperation_t transB, I m, I n, I k, const void* alpha, \
                         const void* A[], hipDataType aType, I lda, const void* B[], hipDataType bType, I ldb, const void* beta, void* C[], \
                         hipDataType cType, I ldc, I batchCount, hipblasComputeType_t computeType,                                      \
                         hipblasGemmAlgo_t algo __VA_OPT__(, hipblasGemmFlags_t) __VA_ARGS__) {                                         \
        hipblasStatus_t st;                                                                                                             \
        if (batched_ptr_gemm(handle, dtype_of(aType, bType, cType, computeType), transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, \
                             batchCount, &st))                                                                                          \
            return st;                                                                                                                  \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, transA, transB, m, n, k, alpha, A, aType, lda, B, bType, ldb, beta, C, \
                   cType, ldc, batchCount, computeType, algo __VA_OPT__(, ) __VA_ARGS__);                                               \
    }
// rocblas_{s,d,c,z}gemm_batched and the _64 twin: act only with GEMMUL8_HOOK_ROCBLAS=1 (rocblas_takes)
#define OZ2_ROCBLAS_PB_HOOK(NAME, T, I, CODE)                                                                                           \
    int NAME(void* handle, int transA, int transB, I m, I n, I k, const T* alpha, const T* const A[], I lda, const T* const B[], I ldb, \
             const T* beta, T* const C[], I ldc, I batchCount) {                                                                        \
        hipStream_t s_;                                                                                                                 \
        hipblasStatus_t st_;                                                                                                            \
        if (tl_native_depth == 0 && rocblas_takes(handle, transA, transB, &s_) &&                                                       \
            batched_ptr_gemm((hipblasHandle_t)handle, CODE, transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, batchCount, &st_, &s_)) \
            return rocblas_status_of(st_);                                                                                              \
        OZ2_NATIVE(NAME, 6, handle, transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc, batchCount);                          \
    }
// the trailing argument, if any, is the `flags` of the WithFlags forms
#define OZ2_GEMM_EX_HOOK(NAME, I, ...)                                                                                                  \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasOperation_t transA, hipblasOperation_t transB, I m, I n, I k, const void* alpha, \
                         const void* A, hipDataType aType, I lda, const void* B, hipDataType bType, I ldb, const void* beta, void* C,   \
                         hipDataType cType, I ldc, hipblasComputeType_t computeType,                                                    \
                         hipblasGemmAlgo_t algo __VA_OPT__(, hipblasGemmFlags_t) __VA_ARGS__) {                                         \
        hipblasStatus_t st;                                                                                                             \
        if (plain_gemm(handle, dtype_of(aType, bType, cType, computeType), transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C,     \
                       ldc, &st))                                                                                                       \
            return st;                                                                                                                  \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, transA, transB, m, n, k, alpha, A, aType, lda, B, bType, ldb, beta, C, \
                   cType, ldc, computeType, algo __VA_OPT__(, ) __VA_ARGS__);                                                           \
    }
// the rocBLAS C entry points: act only with GEMMUL8_HOOK_ROCBLAS=1 (rocblas_takes)
#define OZ2_ROCBLAS_HOOK(NAME, SB_NAME, T, CODE)                                                                                        \
    int NAME(void* handle, int transA, int transB, int m, int n, int k, const T* alpha, const T* A, int lda, const T* B, int ldb,       \
             const T* beta, T* C, int ldc) {                                                                                            \
        GemmCall c;                                                                                                                     \
        hipStream_t s_;                                                                                                                 \
        hipblasStatus_t st_;                                                                                                            \
        if (gemm_call(&c, CODE, transA, transB, m, n, k, alpha, A, lda, 0, B, ldb, 0, beta, C, ldc, 0) && alpha && beta &&              \
            rocblas_takes(handle, transA, transB, &s_) && try_emulate(handle, c, &st_, &s_))                                            \
            return rocblas_status_of(st_);                                                                                              \
        OZ2_NATIVE(NAME, 6, handle, transA, transB, m, n, k, alpha, A, lda, B, ldb, beta, C, ldc);                                      \
    }                                                                                                                                   \
    int SB_NAME(void* handle, int transA, int transB, int m, int n, int k, const T* alpha, const T* A, int lda, long long strideA,      \
                const T* B, int ldb, long long strideB, const T* beta, T* C, int ldc, long long strideC, int batchCount) {              \
        GemmCall c;                                                                                                                     \
        hipStream_t s_;                                                                                                                 \
        hipblasStatus_t st_;                                                                                                            \
        if (gemm_call(&c, CODE, transA, transB, m, n, k, alpha, A, lda, strideA, B, ldb, strideB, beta, C, ldc, strideC, batchCount) && \
            alpha && beta && rocblas_takes(handle, transA, transB, &s_) && emulate_batch(handle, c, &st_, &s_))                         \
            return rocblas_status_of(st_);                                                                                              \
        OZ2_NATIVE(SB_NAME, 6, handle, transA, transB, m, n, k, alpha, A, lda, strideA, B, ldb, strideB, beta, C, ldc, strideC,         \
                   batchCount);                                                                                                         \
    }
// rocblas_internal_gemm_template<T> (I = int) and rocblas_internal_gemm_template_64<T> (I = long) under their mangled names
#define OZ2_ROCBLAS_INTERNAL(FN, T, I, CODE, SYM)                                                                                       \
    int FN(void* h, int ta, int tb, I m, I n, I k, const T* al, const T* A, long oa, I lda, long sa, const T* B, long ob, I ldb, long sb, \
           const T* be, T* C, long oc, I ldc, long sc, I bc) __asm__(SYM);                                                              \
    int FN(void* h, int ta, int tb, I m, I n, I k, const T* al, const T* A, long oa, I lda, long sa, const T* B, long ob, I ldb, long sb, \
           const T* be, T* C, long oc, I ldc, long sc, I bc) {                                                                          \
        static const auto real_ = real<decltype(&FN)>(SYM);                                                                             \
        return rocblas_internal_gemm_hook<T, I>(real_, CODE, h, ta, tb, m, n, k, al, A, oa, lda, sa, B, ob, ldb, sb, be, C, oc, ldc, sc, bc); \
    }
#define OZ2_SYRK_HOOK(NAME, T, I, CODE)                                                                                                 \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasFillMode_t uplo, hipblasOperation_t transA, I n, I k, const T* alpha, const T* A, \
                         I lda, const T* beta, T* C, I ldc) {                                                                           \
        hipblasStatus_t st;                                                                                                             \
        const Level3Call c{.routine = kSYRK, .dtype = CODE, .uplo = (int)uplo, .trans = (int)transA, .n = n, .k = k, .alpha = alpha, .A = A, .lda = lda, \
                           .beta = beta, .C = C, .ldc = ldc};                                                                           \
        if (try_level3(handle, c, &st)) return st;                                                                                      \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, uplo, transA, n, k, alpha, A, lda, beta, C, ldc);                      \
    }
#define OZ2_SYR2K_HOOK(NAME, T, I, CODE)                                                                                                \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasFillMode_t uplo, hipblasOperation_t transA, I n, I k, const T* alpha, const T* A, \
                         I lda, const T* B, I ldb, const T* beta, T* C, I ldc) {                                                        \
        hipblasStatus_t st;                                                                                                             \
        const Level3Call c{.routine = kSYR2K, .dtype = CODE, .uplo = (int)uplo, .trans = (int)transA, .n = n, .k = k, .alpha = alpha, .A = A, .lda = lda, \
                           .B = B, .ldb = ldb, .beta = beta, .C = C, .ldc = ldc};                                                       \
        if (try_level3(handle, c, &st)) return st;                                                                                      \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, uplo, transA, n, k, alpha, A, lda, B, ldb, beta, C, ldc);              \
    }
// hipblas{S,D,C,Z}symm (KIND = kSYMM) and hipblas{C,Z}hemm (kHEMM): one signature
#define OZ2_SYMM_HOOK(NAME, KIND, T, I, CODE)                                                                                           \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasSideMode_t side, hipblasFillMode_t uplo, I m, I n, const T* alpha, const T* A,  \
                         I lda, const T* B, I ldb, const T* beta, T* C, I ldc) {                                                        \
        hipblasStatus_t st;                                                                                                             \
        const Level3Call c{.routine = KIND, .dtype = CODE, .side = (int)side, .uplo = (int)uplo, .m = m, .n = n, .alpha = alpha, .A = A, .lda = lda, \
                           .B = B, .ldb = ldb, .beta = beta, .C = C, .ldc = ldc};                                                       \
        if (try_level3(handle, c, &st)) return st;                                                                                      \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, side, uplo, m, n, alpha, A, lda, B, ldb, beta, C, ldc);                \
    }
// hipblas{S,D,C,Z}trmm: ROCm 7's out-of-place signature (C may be B)
#define OZ2_TRMM_HOOK(NAME, T, I, CODE)                                                                                                 \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasSideMode_t side, hipblasFillMode_t uplo, hipblasOperation_t transA,             \
                         hipblasDiagType_t diag, I m, I n, const T* alpha, const T* A, I lda, const T* B, I ldb, T* C, I ldc) {         \
        hipblasStatus_t st;                                                                                                             \
        const Level3Call c{.routine = kTRMM, .dtype = CODE, .side = (int)side, .uplo = (int)uplo, .trans = (int)transA, .diag = (int)diag, .m = m, .n = n, \
                           .alpha = alpha, .A = A, .lda = lda, .B = B, .ldb = ldb, .C = C, .ldc = ldc};                                 \
        if (try_level3(handle, c, &st)) return st;                                                                                      \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, side, uplo, transA, diag, m, n, alpha, A, lda, B, ldb, C, ldc);        \
    }
// hipblas{S,D,C,Z}trsm: in place on B, the matrix the call writes (Level3Call::C)
#define OZ2_TRSM_HOOK(NAME, T, I, CODE)                                                                                                 \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasSideMode_t side, hipblasFillMode_t uplo, hipblasOperation_t transA,             \
                         hipblasDiagType_t diag, I m, I n, const T* alpha, const T* A, I lda, T* B, I ldb) {                            \
        hipblasStatus_t st;                                                                                                             \
        const Level3Call c{.routine = kTRSM, .dtype = CODE, .side = (int)side, .uplo = (int)uplo, .trans = (int)transA, .diag = (int)diag, .m = m, .n = n, \
                           .alpha = alpha, .A = A, .lda = lda, .C = B, .ldc = ldb};                                                     \
        if (try_level3(handle, c, &st)) return st;                                                                                      \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, side, uplo, transA, diag, m, n, alpha, A, lda, B, ldb);                \
    }
// hipblas{C,Z}her2k: a complex alpha, R = the real type of beta
#define OZ2_HER2K_HOOK(NAME, T, R, I, CODE)                                                                                             \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasFillMode_t uplo, hipblasOperation_t transA, I n, I k, const T* alpha, const T* A, \
                         I lda, const T* B, I ldb, const R* beta, T* C, I ldc) {                                                        \
        hipblasStatus_t st;                                                                                                             \
        const Level3Call c{.routine = kHER2K, .dtype = CODE, .uplo = (int)uplo, .trans = (int)transA, .n = n, .k = k, .alpha = alpha, .A = A, .lda = lda, \
                           .B = B, .ldb = ldb, .beta = beta, .C = C, .ldc = ldc};                                                       \
        if (try_level3(handle, c, &st)) return st;                                                                                      \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, uplo, transA, n, k, alpha, A, lda, B, ldb, beta, C, ldc);              \
    }
// hipblas{C,Z}herk: R = the real type of alpha and beta
#define OZ2_HERK_HOOK(NAME, T, R, I, CODE)                                                                                              \
    hipblasStatus_t NAME(hipblasHandle_t handle, hipblasFillMode_t uplo, hipblasOperation_t transA, I n, I k, const R* alpha, const T* A, \
                         I lda, const R* beta, T* C, I ldc) {                                                                           \
        hipblasStatus_t st;                                                                                                             \
        const Level3Call c{.routine = kHERK, .dtype = CODE, .uplo = (int)uplo, .trans = (int)transA, .n = n, .k = k, .alpha = alpha, .A = A, .lda = lda, \
                           .beta = beta, .C = C, .ldc = ldc};                                                                           \
        if (try_level3(handle, c, &st)) return st;                                                                                      \
        OZ2_NATIVE(NAME, HIPBLAS_STATUS_NOT_INITIALIZED, handle, uplo, transA, n, k, alpha, A, lda, beta, C, ldc);                      \
    }
// one stamp per type; Z / ZZ: the substitution indices of the mangled names, which differ between the real and the complex forms
#define OZ2_TYPE_HOOKS(L, U, T, CODE, TAG, Z, ZZ, ZZZ)                                                                                   \
    OZ2_GEMM_HOOK(hipblas##U##gemm, T, int, CODE)                                                                                       \
    OZ2_GEMM_HOOK(hipblas##U##gemm_64, T, int64_t, CODE)                                                                                \
    OZ2_SB_HOOK(hipblas##U##gemmStridedBatched, T, CODE)                                                                                \
    OZ2_PB_HOOK(hipblas##U##gemmBatched, T, int, CODE)                                                                                  \
    OZ2_PB_HOOK(hipblas##U##gemmBatched_64, T, int64_t, CODE)                                                                           \
    OZ2_ROCBLAS_PB_HOOK(rocblas_##L##gemm_batched, T, int, CODE)                                                                        \
    OZ2_ROCBLAS_PB_HOOK(rocblas_##L##gemm_batched_64, T, int64_t, CODE)                                                                 \
    OZ2_SYRK_HOOK(hipblas##U##syrk, T, int, CODE)                                                                                       \
    OZ2_SYRK_HOOK(hipblas##U##syrk_64, T, int64_t, CODE)                                                                                \
    OZ2_SYR2K_HOOK(hipblas##U##syr2k, T, int, CODE)                                                                                     \
    OZ2_SYR2K_HOOK(hipblas##U##syr2k_64, T, int64_t, CODE)                                                                              \
    OZ2_SYMM_HOOK(hipblas##U##symm, kSYMM, T, int, CODE)                                                                                \
    OZ2_SYMM_HOOK(hipblas##U##symm_64, kSYMM, T, int64_t, CODE)                                                                         \
    OZ2_TRMM_HOOK(hipblas##U##trmm, T, int, CODE)                                                                                       \
    OZ2_TRMM_HOOK(hipblas##U##trmm_64, T, int64_t, CODE)                                                                                \
    OZ2_TRSM_HOOK(hipblas##U##trsm, T, int, CODE)                                                                                       \
    OZ2_TRSM_HOOK(hipblas##U##trsm_64, T, int64_t, CODE)                                                                                \
    OZ2_ROCBLAS_HOOK(rocblas_##L##gemm, rocblas_##L##gemm_strided_batched, T, CODE)                                                     \
    OZ2_ROCBLAS_INTERNAL(oz2_rb_int_gemm_##L##_32, T, int, CODE,                                                                        \
                         "_Z30rocblas_internal_gemm_templateI" TAG "E15rocblas_status_P15_rocblas_handle18rocblas_operation_" Z         \
                         "_iiiPKT_" ZZ "_lil" ZZ "_lil" ZZ "_P" ZZZ "_lili")                                                            \
    OZ2_ROCBLAS_INTERNAL(oz2_rb_int_gemm_##L##_64, T, long, CODE,                                                                       \
                         "_Z33rocblas_internal_gemm_template_64I" TAG "E15rocblas_status_P15_rocblas_handle18rocblas_operation_" Z      \
                         "_lllPKT_" ZZ "_lll" ZZ "_lll" ZZ "_P" ZZZ "_llll")
OZ2_TYPE_HOOKS(s, S, float, GEMMUL8_S, "f", "S3", "S6", "S4")
OZ2_TYPE_HOOKS(d, D, double, GEMMUL8_D, "d", "S3", "S6", "S4")
OZ2_TYPE_HOOKS(c, C, hipComplex, GEMMUL8_C, "19rocblas_complex_numIfE", "S5", "S8", "S6")
OZ2_TYPE_HOOKS(z, Z, hipDoubleComplex, GEMMUL8_Z, "19rocblas_complex_numIdE", "S5", "S8", "S6")
OZ2_HERK_HOOK(hipblasCherk, hipComplex, float, int, GEMMUL8_C)
OZ2_HERK_HOOK(hipblasCherk_64, hipComplex, float, int64_t, GEMMUL8_C)
OZ2_HERK_HOOK(hipblasZherk, hipDoubleComplex, double, int, GEMMUL8_Z)
OZ2_HERK_HOOK(hipblasZherk_64, hipDoubleComplex, double, int64_t, GEMMUL8_Z)
OZ2_HER2K_HOOK(hipblasCher2k, hipComplex, float, int, GEMMUL8_C)
OZ2_HER2K_HOOK(hipblasCher2k_64, hipComplex, float, int64_t, GEMMUL8_C)
OZ2_HER2K_HOOK(hipblasZher2k, hipDoubleComplex, double, int, GEMMUL8_Z)
OZ2_HER2K_HOOK(hipblasZher2k_64, hipDoubleComplex, double, int64_t, GEMMUL8_Z)
OZ2_SYMM_HOOK(hipblasChemm, kHEMM, hipComplex, int, GEMMUL8_C)
OZ2_SYMM_HOOK(hipblasChemm_64, kHEMM, hipComplex, int64_t, GEMMUL8_C)
OZ2_SYMM_HOOK(hipblasZhemm, kHEMM, hipDoubleComplex, int, GEMMUL8_Z)
OZ2_SYMM_HOOK(hipblasZhemm_64, kHEMM, hipDoubleComplex, int64_t, GEMMUL8_Z)
OZ2_GEMM_EX_HOOK(hipblasGemmEx, int)
OZ2_GEMM_EX_HOOK(hipblasGemmEx_64, int64_t)
OZ2_GEMM_EX_HOOK(hipblasGemmExWithFlags, int, flags)
OZ2_GEMM_EX_HOOK(hipblasGemmExWithFlags_64, int64_t, flags)
OZ2_PB_EX_HOOK(hipblasGemmBatchedEx, int)
OZ2_PB_EX_HOOK(hipblasGemmBatchedEx_64, int64_t)
OZ2_PB_EX_HOOK(hipblasGemmBatchedExWithFlags, int, flags)
OZ2_PB_EX_HOOK(hipblasGemmBatchedExWithFlags_64, int64_t, flags)
#undef OZ2_TYPE_HOOKS
#undef OZ2_ROCBLAS_INTERNAL
#undef OZ2_ROCBLAS_HOOK
#undef OZ2_GEMM_EX_HOOK
#undef OZ2_ROCBLAS_PB_HOOK
#undef OZ2_PB_EX_HOOK
#undef OZ2_PB_HOOK
#undef OZ2_HERK_HOOK
#undef OZ2_HER2K_HOOK
#undef OZ2_SYMM_HOOK
#undef OZ2_TRMM_HOOK
#undef OZ2_TRSM_HOOK
#undef OZ2_SYR2K_HOOK
#undef OZ2_SYRK_HOOK
#undef OZ2_SB_HOOK
#undef OZ2_GEMM_HOOK

hipblasStatus_t hipblasGemmStridedBatchedEx(hipblasHandle_t handle, hipblasOperation_t transA, hipblasOperation_t transB, int m, int n, int k,
                                            const void* alpha, const void* A, hipDataType aType, int lda, hipblasStride strideA, const void* B,
                                            hipDataType bType, int ldb, hipblasStride strideB, const void* beta, void* C, hipDataType cType,
                                            int ldc, hipblasStride strideC, int batchCount, hipblasComputeType_t computeType,
                                            hipblasGemmAlgo_t algo) {
    hipblasStatus_t st;
    if (batched_gemm(handle, dtype_of(aType, bType, cType, computeType), transA, transB, m, n, k, alpha, A, lda, strideA, B, ldb, strideB, beta, C, ldc,
                     strideC, batchCount, &st))
        return st;
    OZ2_NATIVE(hipblasGemmStridedBatchedEx, HIPBLAS_STATUS_NOT_INITIALIZED, handle, transA, transB, m, n, k, alpha, A, aType, lda, strideA, B, bType, ldb,
               strideB, beta, C, cType, ldc, strideC, batchCount, computeType, algo);
}

int rocblas_destroy_handle(void* handle) {
    if (handle) release_state((hipblasHandle_t)handle, true);
    OZ2_NATIVE(rocblas_destroy_handle, 6, handle);
}
// rocblas_gemm_ex: D = alpha op(A) op(B) + beta C.  Emulated for the four plain types (all of a / b / c / d / compute the same type) when it
// is the in-place form (c == d, ldc == ldd) -- what rocBLAS's own clients and hipBLAS's GemmEx issue; anything else goes to rocBLAS.
int rocblas_gemm_ex(void* handle, int transA, int transB, int m, int n, int k, const void* alpha, const void* a, int a_type, int lda,
                    const void* b, int b_type, int ldb, const void* beta, const void* c, int c_type, int ldc, void* d, int d_type, int ldd,
                    int compute_type, int algo, int32_t solution_index, uint32_t flags) {
    const bool same = a_type == b_type && b_type == c_type && c_type == d_type && d_type == compute_type;
    GemmCall g;
    hipStream_t s_;
    hipblasStatus_t st_;
    if (same && c == d && ldc == ldd && gemm_call(&g, dtype_of_rocblas(a_type), transA, transB, m, n, k, alpha, a, lda, 0, b, ldb, 0, beta, d, ldd, 0) &&
        alpha && beta && rocblas_takes(handle, transA, transB, &s_) && try_emulate(handle, g, &st_, &s_))
        return rocblas_status_of(st_);
    OZ2_NATIVE(rocblas_gemm_ex, 6, handle, transA, transB, m, n, k, alpha, a, a_type, lda, b, b_type, ldb, beta, c, c_type, ldc, d, d_type, ldd, compute_type,
               algo, solution_index, flags);
}

// rocblas_gemm_batched_ex: the pointer-array twin of rocblas_gemm_ex, under the same conditions (one plain type, the in-place form c == d, ldc == ldd)
int rocblas_gemm_batched_ex(void* handle, int transA, int transB, int m, int n, int k, const void* alpha, const void* a, int a_type, int lda,
                            const void* b, int b_type, int ldb, const void* beta, const void* c, int c_type, int ldc, void* d, int d_type, int ldd,
                            int batch_count, int compute_type, int algo, int32_t solution_index, uint32_t flags) {
    const bool same = a_type == b_type && b_type == c_type && c_type == d_type && d_type == compute_type;
    hipStream_t s_;
    hipblasStatus_t st_;
    if (same && c == d && ldc == ldd && tl_native_depth == 0 && rocblas_takes(handle, transA, transB, &s_) &&
        batched_ptr_gemm((hipblasHandle_t)handle, dtype_of_rocblas(a_type), transA, transB, m, n, k, alpha, a, lda, b, ldb, beta, d, ldd, batch_count, &st_, &s_))
        return rocblas_status_of(st_);
    OZ2_NATIVE(rocblas_gemm_batched_ex, 6, handle, transA, transB, m, n, k, alpha, a, a_type, lda, b, b_type, ldb, beta, c, c_type, ldc, d, d_type, ldd,
               batch_count, compute_type, algo, solution_index, flags);
}

hipblasStatus_t hipblasLtMatrixLayoutCreate(hipblasLtMatrixLayout_t* matLayout, hipDataType type, uint64_t rows, uint64_t cols, int64_t ld) {
    OZ2_REAL(hipblasLtMatrixLayoutCreate);
    if (!real_) return HIPBLAS_STATUS_NOT_INITIALIZED;
    const hipblasStatus_t st = real_(matLayout, type, rows, cols, ld);
    if (st == HIPBLAS_STATUS_SUCCESS && matLayout && *matLayout) {
        LtLayout rec;
        rec.type = (int32_t)type, rec.order = HIPBLASLT_ORDER_COL, rec.batch = 1, rec.rows = rows, rec.cols = cols, rec.ld = ld;
        std::lock_guard<std::mutex> g(g_lt_mtx);
        g_lt_layouts[*matLayout] = rec;
    }
    return st;
}
hipblasStatus_t hipblasLtMatrixLayoutSetAttribute(hipblasLtMatrixLayout_t matLayout, hipblasLtMatrixLayoutAttribute_t attr, const void* buf,
                                                  size_t sizeInBytes) {
    OZ2_REAL(hipblasLtMatrixLayoutSetAttribute);
    if (!real_) return HIPBLAS_STATUS_NOT_INITIALIZED;
    const hipblasStatus_t st = real_(matLayout, attr, buf, sizeInBytes);
    if (st == HIPBLAS_STATUS_SUCCESS && buf) {
        std::lock_guard<std::mutex> g(g_lt_mtx);
        auto it = g_lt_layouts.find(matLayout);
        if (it != g_lt_layouts.end()) {
            LtLayout& r = it->second;
            switch (attr) {
            case HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT: if (sizeInBytes >= 4) std::memcpy(&r.batch, buf, 4); break;
            case HIPBLASLT_MATRIX_LAYOUT_STRIDED_BATCH_OFFSET: if (sizeInBytes >= 8) std::memcpy(&r.stride, buf, 8); break;
            case HIPBLASLT_MATRIX_LAYOUT_TYPE: if (sizeInBytes >= 4) std::memcpy(&r.type, buf, 4); break;
            case HIPBLASLT_MATRIX_LAYOUT_ORDER: if (sizeInBytes >= 4) std::memcpy(&r.order, buf, 4); break;
            case HIPBLASLT_MATRIX_LAYOUT_ROWS: if (sizeInBytes >= 8) std::memcpy(&r.rows, buf, 8); break;
            case HIPBLASLT_MATRIX_LAYOUT_COLS: if (sizeInBytes >= 8) std::memcpy(&r.cols, buf, 8); break;
            case HIPBLASLT_MATRIX_LAYOUT_LD: if (sizeInBytes >= 8) std::memcpy(&r.ld, buf, 8); break;
            default: break;
            }
        }
    }
    return st;
}
hipblasStatus_t hipblasLtMatrixLayoutDestroy(const hipblasLtMatrixLayout_t matLayout) {
    {
        std::lock_guard<std::mutex> g(g_lt_mtx);
        g_lt_layouts.erase(matLayout);
    }
    OZ2_NATIVE(hipblasLtMatrixLayoutDestroy, HIPBLAS_STATUS_NOT_INITIALIZED, matLayout);
}
// the per-handle state of an hipblasLt handle is released with the handle, as for hipblasDestroy
hipblasStatus_t hipblasLtDestroy(const hipblasLtHandle_t handle) {
    release_state((hipblasHandle_t)handle, true);
    OZ2_NATIVE(hipblasLtDestroy, HIPBLAS_STATUS_NOT_INITIALIZED, handle);
}
hipblasStatus_t hipblasLtMatmul(hipblasLtHandle_t handle, hipblasLtMatmulDesc_t matmulDesc, const void* alpha, const void* A,
                                hipblasLtMatrixLayout_t Adesc, const void* B, hipblasLtMatrixLayout_t Bdesc, const void* beta, const void* C,
                                hipblasLtMatrixLayout_t Cdesc, void* D, hipblasLtMatrixLayout_t Ddesc, const hipblasLtMatmulAlgo_t* algo, void* workspace,
                                size_t workspaceSizeInBytes, hipStream_t stream) {
    hipblasStatus_t st;
    if (lt_try(handle, matmulDesc, alpha, A, Adesc, B, Bdesc, beta, C, Cdesc, D, Ddesc, stream, &st)) return st;
    OZ2_NATIVE(hipblasLtMatmul, HIPBLAS_STATUS_NOT_INITIALIZED, handle, matmulDesc, alpha, A, Adesc, B, Bdesc, beta, C, Cdesc, D, Ddesc, algo, workspace,
               workspaceSizeInBytes, stream);
}

}  // extern "C"
#pragma GCC visibility pop
