// Characterises the Level-3 gates of the LD_PRELOAD hook (gemmul8_amd/csrc/oz2_hook.cpp: hipblas?syrk / herk / syr2k / her2k / symm / hemm / trmm /
// trsm and the _64 twins, 52 entry points) against mock_gpu.cpp + mock_level3.cpp: one scenario per process (argv[1]; the hook's once-only notices and
// its cached GEMMUL8_HOOK_STATS / GEMMUL8_NONFINITE reads are per process).  What the run prints -- this program's "call" / "->" lines, the mock's
// "native" / "abi" lines and the hook's notices and statistics -- is the transcript tests/test_hook_level3_gate.py compares with
// tests/golden/hook_level3_transcript.json.  Linked against the natives-only build of mock_level3.cpp for the scenario no-entry.
// The mocks never dereference a matrix: the dimensions are far larger than the three 4 KiB buffers, large enough for the TFLOP figures of the
// statistics to show three digits.
#include <hip/hip_runtime.h>
#include <hipblas/hipblas.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

extern "C" {
hipblasStatus_t mock_create(hipblasHandle_t*);
void mock_level3_register(const char* name, const void* base, size_t bytes);
}

namespace {
enum { kSYRK, kHERK, kSYR2K, kHER2K, kSYMM, kHEMM, kTRMM, kTRSM, kRoutines };
constexpr int L = HIPBLAS_SIDE_LEFT, R = HIPBLAS_SIDE_RIGHT, UP = HIPBLAS_FILL_MODE_UPPER, LO = HIPBLAS_FILL_MODE_LOWER, N = HIPBLAS_OP_N, T = HIPBLAS_OP_T,
              C = HIPBLAS_OP_C, NU = HIPBLAS_DIAG_NON_UNIT;
alignas(16) char g_A[4096], g_B[4096], g_C[4096];

struct Args {
    int side = L, uplo = UP, trans = N, diag = NU;
    long long m = 0, n = 0, k = 0, lda = 0, ldb = 0, ldc = 0;
    double ar = 1, ai = 0, br = 0, bi = 0;
    bool alpha = true, beta = true, A = true, B = true, C = true;  // false: a null pointer
    size_t offA = 0, offB = 0, offC = 0;                           // bytes
};
template <typename S> S scalar(double re, double im);
template <> float scalar<float>(double re, double) { return (float)re; }
template <> double scalar<double>(double re, double) { return re; }
template <> hipComplex scalar<hipComplex>(double re, double im) { return make_hipFloatComplex((float)re, (float)im); }
template <> hipDoubleComplex scalar<hipDoubleComplex>(double re, double im) { return make_hipDoubleComplex(re, im); }

using Call = std::function<hipblasStatus_t(hipblasHandle_t, const Args&)>;
#define FILL (hipblasFillMode_t) a.uplo
#define SIDE (hipblasSideMode_t) a.side
#define OP (hipblasOperation_t) a.trans
#define DIAG (hipblasDiagType_t) a.diag
#define PA (a.A ? (const E*)(g_A + a.offA) : nullptr)
#define PB (a.B ? (E*)(g_B + a.offB) : nullptr)
#define PC (a.C ? (E*)(g_C + a.offC) : nullptr)
#define SCALARS(SA, SB)                                                    \
    const SA al_ = scalar<SA>(a.ar, a.ai);                                 \
    const SB be_ = scalar<SB>(a.br, a.bi);                                 \
    const SA* const al = a.alpha ? &al_ : nullptr;                         \
    const SB* const be = a.beta ? &be_ : nullptr;                          \
    (void)be
// syrk (S = E) and herk (S = the real type)
template <typename E, typename S, typename I>
Call wrap(hipblasStatus_t (*f)(hipblasHandle_t, hipblasFillMode_t, hipblasOperation_t, I, I, const S*, const E*, I, const S*, E*, I)) {
    return [f](hipblasHandle_t h, const Args& a) {
        SCALARS(S, S);
        return f(h, FILL, OP, (I)a.n, (I)a.k, al, PA, (I)a.lda, be, PC, (I)a.ldc);
    };
}
// syr2k (S = E), her2k (S = the real type, beta only) -- and symm / hemm, whose signature differs in the enums' types alone
template <typename E, typename S, typename I>
Call wrap(hipblasStatus_t (*f)(hipblasHandle_t, hipblasFillMode_t, hipblasOperation_t, I, I, const E*, const E*, I, const E*, I, const S*, E*, I)) {
    return [f](hipblasHandle_t h, const Args& a) {
        SCALARS(E, S);
        return f(h, FILL, OP, (I)a.n, (I)a.k, al, PA, (I)a.lda, PB, (I)a.ldb, be, PC, (I)a.ldc);
    };
}
template <typename E, typename I>
Call wrap(hipblasStatus_t (*f)(hipblasHandle_t, hipblasSideMode_t, hipblasFillMode_t, I, I, const E*, const E*, I, const E*, I, const E*, E*, I)) {
    return [f](hipblasHandle_t h, const Args& a) {
        SCALARS(E, E);
        return f(h, SIDE, FILL, (I)a.m, (I)a.n, al, PA, (I)a.lda, PB, (I)a.ldb, be, PC, (I)a.ldc);
    };
}
template <typename E, typename I>
Call wrap(hipblasStatus_t (*f)(hipblasHandle_t, hipblasSideMode_t, hipblasFillMode_t, hipblasOperation_t, hipblasDiagType_t, I, I, const E*, const E*, I,
                               const E*, I, E*, I)) {
    return [f](hipblasHandle_t h, const Args& a) {
        SCALARS(E, E);
        return f(h, SIDE, FILL, OP, DIAG, (I)a.m, (I)a.n, al, PA, (I)a.lda, PB, (I)a.ldb, PC, (I)a.ldc);
    };
}
template <typename E, typename I>
Call wrap(hipblasStatus_t (*f)(hipblasHandle_t, hipblasSideMode_t, hipblasFillMode_t, hipblasOperation_t, hipblasDiagType_t, I, I, const E*, const E*, I, E*, I)) {
    return [f](hipblasHandle_t h, const Args& a) {
        SCALARS(E, E);
        return f(h, SIDE, FILL, OP, DIAG, (I)a.m, (I)a.n, al, PA, (I)a.lda, PB, (I)a.ldb);
    };
}

struct Entry {
    const char* name;
    int routine;
    char type;  // S, D, C, Z
    bool ilp64;
    Call call;
};
#define E2(NAME, ROUTINE, TYPE) {#NAME, ROUTINE, TYPE, false, wrap(NAME)}, {#NAME "_64", ROUTINE, TYPE, true, wrap(NAME##_64)}
#define TYPE_ENTRIES(U) \
    E2(hipblas##U##syrk, kSYRK, #U[0]), E2(hipblas##U##syr2k, kSYR2K, #U[0]), E2(hipblas##U##symm, kSYMM, #U[0]), E2(hipblas##U##trmm, kTRMM, #U[0]), \
        E2(hipblas##U##trsm, kTRSM, #U[0])
#define HERM_ENTRIES(U) E2(hipblas##U##herk, kHERK, #U[0]), E2(hipblas##U##her2k, kHER2K, #U[0]), E2(hipblas##U##hemm, kHEMM, #U[0])
const std::vector<Entry> kEntries = {TYPE_ENTRIES(S), TYPE_ENTRIES(D), TYPE_ENTRIES(C), TYPE_ENTRIES(Z), HERM_ENTRIES(C), HERM_ENTRIES(Z)};

const Entry& entry(const char* name) {
    for (const Entry& e : kEntries)
        if (!std::strcmp(e.name, name)) return e;
    std::printf("no entry point %s\n", name);
    std::exit(2);
}
// the 32-bit S form of a routine, the C form of the three Hermitian ones
const Entry& first_of(int routine, bool ilp64 = false) {
    for (const Entry& e : kEntries)
        if (e.routine == routine && e.ilp64 == ilp64) return e;
    std::exit(2);
}
bool hermitian(int routine) { return routine == kHERK || routine == kHER2K || routine == kHEMM; }

// one hooked call on a handle of its own, destroyed afterwards: every call's workspace is sized from nothing
void run(const Entry& e, const Args& a, const char* note = "") {
    std::printf("call %s%s%s\n", e.name, *note ? " : " : "", note);
    hipblasHandle_t h;
    mock_create(&h);
    const hipblasStatus_t st = e.call(h, a);
    std::printf("  -> status %d\n", (int)st);
    if (hipblasDestroy(h) != HIPBLAS_STATUS_SUCCESS) std::printf("  hipblasDestroy failed\n");
}
// the i-th distinct call: shape, leading dimensions, enums (valid for the routine), scalars and offsets all depend on i
Args nth(const Entry& e, int i) {
    Args a;
    a.m = 3000 + 101 * i, a.n = 4100 + 67 * i, a.k = 5200 + 89 * i;
    a.lda = 9000 + i, a.ldb = 9100 + i, a.ldc = 9200 + i;
    a.uplo = i % 2 ? UP : LO;
    a.side = (i / 2) % 2 ? L : R;
    a.diag = NU + (i / 4) % 2;
    if (e.routine <= kHER2K) a.trans = (i / 2) % 2 ? N : hermitian(e.routine) ? C : T;
    else a.trans = N + i % 3;
    a.ar = 1 + 0.25 * i, a.ai = 0.5 * i, a.br = 2 - 0.125 * i, a.bi = -0.25 * i;
    a.offA = 16 * (i % 7), a.offB = 16 * (i % 5), a.offC = 16 * (i % 3);
    return a;
}
void every_entry_point() {
    int i = 0;
    for (const Entry& e : kEntries) run(e, nth(e, i)), ++i;
}
void select_all() {
    setenv("GEMMUL8_NUM_MOD_S", "8", 1), setenv("GEMMUL8_NUM_MOD_D", "15", 1), setenv("GEMMUL8_NUM_MOD_C", "7", 1), setenv("GEMMUL8_NUM_MOD_Z", "14", 1);
    setenv("GEMMUL8_FASTMODE_C", "1", 1);
}
void set_floor(double flops) {
    char buf[32];
    std::snprintf(buf, sizeof buf, "%.0f", flops);
    setenv("GEMMUL8_MIN_FLOPS", buf, 1);
    std::printf("GEMMUL8_MIN_FLOPS=%s\n", buf);
}
// the routine's flop count as the floor takes it
double floor_count(int routine, const Args& a) {
    const double m = (double)a.m, n = (double)a.n, k = (double)a.k, ka = a.side == L ? m : n;
    switch (routine) {
    case kSYRK: case kHERK: return n * (n + 1) * k;
    case kSYR2K: return 2 * n * (n + 1) * k;
    case kHER2K: return 8 * n * (n + 1) * k;
    case kSYMM: case kHEMM: return 2 * m * n * ka;
    default: return m * n * ka;
    }
}

void scenario_all() {
    select_all();
    every_entry_point();
    int i = 60;
    for (const char* name : {"hipblasDsyrk", "hipblasZher2k", "hipblasDsymm", "hipblasDtrmm", "hipblasDtrsm"}) run(entry(name), nth(entry(name), i)), ++i;
}
void scenario_moduli_range() {
    setenv("GEMMUL8_NUM_MOD_S", "14", 1);
    int i = 0;
    for (int routine : {kSYRK, kSYR2K, kSYMM, kTRMM, kTRSM})
        for (int rep = 0; rep < 2; ++rep) run(first_of(routine), nth(first_of(routine), i)), ++i;
}
void scenario_limit() {
    setenv("GEMMUL8_NUM_MOD_S", "2", 1), setenv("GEMMUL8_NUM_MOD_C", "2", 1);  // two moduli: the workspaces of the order-2^17 calls stay below 2^37 bytes
    int i = 0;
    for (int routine : {kSYRK, kHERK, kSYR2K, kHER2K})
        for (int over = 0; over < 2; ++over) {
            Args a = nth(first_of(routine), i++);
            a.n = 3 + routine, a.k = (routine == kSYR2K ? 65536 : 131072) + over;
            run(first_of(routine), a, over ? "k above the limit" : "k at the limit");
        }
    for (int routine : {kSYMM, kHEMM, kTRMM, kTRSM})
        for (int side : {L, R})
            for (int over = 0; over < 2; ++over) {
                Args a = nth(first_of(routine), i++);
                a.side = side;
                (side == L ? a.m : a.n) = 131072 + over, (side == L ? a.n : a.m) = 2 + routine;
                run(first_of(routine), a, over ? "order above the limit" : "order at the limit");
            }
}
void scenario_ieee() {
    select_all();
    setenv("GEMMUL8_NONFINITE", "ieee", 1);
    every_entry_point();
    // one GEMM, which is emulated under `ieee`: the mode reaches the library
    static double a[4], b[4], c[4];
    const double one = 1, zero = 0;
    hipblasHandle_t h;
    mock_create(&h);
    std::printf("call hipblasDgemm\n  -> status %d\n", (int)hipblasDgemm(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 2, 2, 2, &one, a, 2, b, 2, &zero, c, 2));
    hipblasDestroy(h);
}
void scenario_floor_number() {
    select_all();
    int i = 0;
    for (int routine = 0; routine < kRoutines; ++routine)
        for (int side : {L, R}) {
            if (routine <= kHER2K && side == R) continue;
            Args a = nth(first_of(routine), i++);
            a.m = 37 + routine, a.n = 53 + 2 * routine, a.k = 29 + 3 * routine, a.side = side;
            const double count = floor_count(routine, a);
            set_floor(count);
            run(first_of(routine), a, "the floor is the call's count: emulated");
            set_floor(count + 1);
            run(first_of(routine), a, "the floor is one above: declined");
        }
}
// the shapes the model accepts were found with gemmul8_hook_would_emulate (GEMMUL8_MIN_FLOPS=auto) at the type's moduli count of select_all
void scenario_floor_auto() {
    select_all();
    setenv("GEMMUL8_MIN_FLOPS", "auto", 1);
    int i = 0;
    for (const char* name : {"hipblasDsyrk", "hipblasZherk", "hipblasDsyr2k", "hipblasZher2k", "hipblasDsymm", "hipblasZhemm", "hipblasDtrmm"})
        for (int side : {L, R})
            for (int big = 0; big < 2; ++big) {
                const Entry& e = entry(name);
                if (e.routine <= kHER2K && side == R) continue;
                Args a = nth(e, i++);
                a.side = side;
                a.m = big ? (side == L ? 8192 : 6144) : 96, a.n = big ? (side == L ? 6144 : 8192) : 64, a.k = big ? (e.routine == kSYR2K ? 4096 : 8192) : 128;
                if (e.routine <= kHER2K) a.n = big ? 8192 : 64;
                run(e, a, big ? "a shape the model accepts" : "a shape the model declines");
            }
    for (int side : {L, R})
        for (int order : {16383, 16384}) {
            Args a = nth(entry("hipblasDtrsm"), i++);
            a.side = side;
            (side == L ? a.m : a.n) = order, (side == L ? a.n : a.m) = 5;
            run(entry("hipblasDtrsm"), a, order < 16384 ? "an order `auto` declines" : "an order `auto` accepts");
        }
}
void scenario_screens() {
    select_all();
    int i = 0;
    for (int routine = 0; routine < kRoutines; ++routine) {
        const Entry& e = first_of(routine);
        const bool rank = routine <= kHER2K, two = routine == kSYR2K || routine == kHER2K, tri = routine == kTRMM || routine == kTRSM;
        const Args base = nth(e, i++);
        Args a;
        // an empty call and a null pointer are the native routine's to answer, uncounted
        for (long long Args::*dim : {&Args::m, &Args::n, &Args::k}) {
            if (rank ? dim == &Args::m : dim == &Args::k) continue;
            a = base, a.*dim = 0;
            run(e, a, dim == &Args::m ? "m = 0" : dim == &Args::n ? "n = 0" : "k = 0");
        }
        a = base, a.alpha = false, run(e, a, "alpha null");
        if (!tri) a = base, a.beta = false, run(e, a, "beta null");
        a = base, a.A = false, run(e, a, "A null");
        if (routine != kSYRK && routine != kHERK) a = base, a.B = false, run(e, a, "B null");
        if (routine != kTRSM) a = base, a.C = false, run(e, a, "C null");
        // an enum out of range is the native routine's too, counted as a native call
        for (int v : {0, (int)HIPBLAS_FILL_MODE_FULL}) a = base, a.uplo = v, run(e, a, v ? "uplo = full" : "uplo = 0");
        if (!rank)
            for (int v : {0, (int)HIPBLAS_SIDE_BOTH}) a = base, a.side = v, run(e, a, v ? "side = both" : "side = 0");
        if (rank || tri)
            for (int v : {0, 114}) a = base, a.trans = v, run(e, a, v ? "trans = 114" : "trans = 0");  // below and just above the defined values
        if (rank) a = base, a.trans = hermitian(routine) ? T : C, run(e, a, hermitian(routine) ? "trans = T" : "trans = C");
        if (tri)
            for (int v : {0, 133}) a = base, a.diag = v, run(e, a, v ? "diag = 133" : "diag = 0");
        // the ILP64 form with a dimension or a leading dimension an int cannot hold
        const Entry& e64 = first_of(routine, true);
        const long long big = 2147483648LL;
        for (long long Args::*dim : {&Args::m, &Args::n, &Args::k, &Args::lda, &Args::ldb, &Args::ldc}) {
            if (rank ? dim == &Args::m : dim == &Args::k) continue;
            if (dim == &Args::ldb && rank && !two) continue;
            if (dim == &Args::ldc && routine == kTRSM) continue;
            a = base, a.*dim = big;
            run(e64, a, dim == &Args::m ? "m = 2^31" : dim == &Args::n ? "n = 2^31" : dim == &Args::k ? "k = 2^31" : dim == &Args::lda ? "lda = 2^31"
                        : dim == &Args::ldb ? "ldb = 2^31" : "ldc = 2^31");
        }
        a = base, run(e64, a, "every dimension fits an int");
    }
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) return std::printf("usage: level3_driver SCENARIO\n"), 2;
    std::setvbuf(stdout, nullptr, _IONBF, 0);  // in order with the hook's stderr
    for (const char* v : {"GEMMUL8_NUM_MOD_S", "GEMMUL8_NUM_MOD_D", "GEMMUL8_NUM_MOD_C", "GEMMUL8_NUM_MOD_Z", "GEMMUL8_FASTMODE_S", "GEMMUL8_FASTMODE_D",
                          "GEMMUL8_FASTMODE_C", "GEMMUL8_FASTMODE_Z", "GEMMUL8_BACKEND", "GEMMUL8_MIN_FLOPS", "GEMMUL8_NONFINITE", "GEMMUL8_SKIP_SCALE_A",
                          "GEMMUL8_SKIP_SCALE_B", "GEMMUL8_MAX_M", "GEMMUL8_MAX_N", "GEMMUL8_MAX_K", "GEMMUL8_MAX_NUM_MOD", "GEMMUL8_MAXWS_BACKEND", "GEMMUL8_DIST",
                          "GEMMUL8_FP8_BOUND", "MOCK_LEVEL3_RC"})
        unsetenv(v);
    setenv("GEMMUL8_HOOK_STATS", "1", 1);
    mock_level3_register("A", g_A, sizeof g_A), mock_level3_register("B", g_B, sizeof g_B), mock_level3_register("C", g_C, sizeof g_C);
    const std::string s = argv[1];
    if (s == "all") scenario_all();
    else if (s == "unselected") every_entry_point();
    else if (s == "moduli-range") scenario_moduli_range();
    else if (s == "fp8") select_all(), setenv("GEMMUL8_BACKEND", "1", 1), every_entry_point();
    else if (s == "limit") scenario_limit();
    else if (s == "ieee") scenario_ieee();
    else if (s == "floor-number") scenario_floor_number();
    else if (s == "floor-auto") scenario_floor_auto();
    else if (s == "declined") select_all(), setenv("MOCK_LEVEL3_RC", "-2", 1), every_entry_point();  // GEMMUL8_E_ARG
    else if (s == "failed") select_all(), setenv("MOCK_LEVEL3_RC", "700", 1), every_entry_point();   // a hipError_t
    else if (s == "screens") scenario_screens();
    else if (s == "no-entry") select_all(), every_entry_point();
    else return std::printf("unknown scenario %s\n", argv[1]), 2;
    return 0;
}
