// Drives every entry point of the LD_PRELOAD hook (gemmul8_amd/csrc/oz2_hook.cpp, built with ASan + UBSan) against the mock
// libraries of mock_gpu.cpp: growing shapes, stream switches, the skip-scaling cache, type switches, the ILP64 / Ex / batched /
// hipblasLt / rocBLAS forms (the internal template by its mangled names), calls outside the emulator's range, the size floor, hipblasDestroy, and several host threads with their own handles.
#include <hip/hip_runtime.h>
#include <hipblas/hipblas.h>
#include <hipblaslt/hipblaslt.h>

#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

extern "C" {
long mock_native_calls();
long mock_emulated_calls();
long mock_live_allocs();
hipblasStatus_t mock_create(hipblasHandle_t*);
hipblasStatus_t mock_set_stream(hipblasHandle_t, hipStream_t);
void* mock_lt_desc(int, int, unsigned);
void* mock_lt_desc_bias(int, int, const void*, int);
void mock_lt_free_desc(void*);
// rocBLAS as oz2_hook.cpp interposes it: plain ints for rocblas_operation / rocblas_datatype / rocblas_status, void* for the handle
int rocblas_destroy_handle(void*);
int rocblas_gemm_ex(void*, int, int, int, int, int, const void*, const void*, int, int, const void*, int, int, const void*, const void*, int, int, void*, int,
                    int, int, int, int32_t, uint32_t);
#define ROCBLAS_DECL(LETTER, T, SYM32, SYM64)                                                                                              \
    int rocblas_##LETTER##gemm(void*, int, int, int, int, int, const T*, const T*, int, const T*, int, const T*, T*, int);                 \
    int rocblas_##LETTER##gemm_strided_batched(void*, int, int, int, int, int, const T*, const T*, int, long long, const T*, int, long long, const T*, T*, \
                                               int, long long, int);                                                                      \
    int rb_int_##LETTER##_32(void*, int, int, int, int, int, const T*, const T*, long, int, long, const T*, long, int, long, const T*, T*, long, int, long, \
                             int) __asm__(SYM32);                                                                                         \
    int rb_int_##LETTER##_64(void*, int, int, long, long, long, const T*, const T*, long, long, long, const T*, long, long, long, const T*, T*, long, long, \
                             long, long) __asm__(SYM64);
// rocblas_internal_gemm_template<T> / _64, called by their mangled names as rocSOLVER does
ROCBLAS_DECL(s, float,
             "_Z30rocblas_internal_gemm_templateIfE15rocblas_status_P15_rocblas_handle18rocblas_operation_S3_iiiPKT_S6_lilS6_lilS6_PS4_lili",
             "_Z33rocblas_internal_gemm_template_64IfE15rocblas_status_P15_rocblas_handle18rocblas_operation_S3_lllPKT_S6_lllS6_lllS6_PS4_llll")
ROCBLAS_DECL(d, double,
             "_Z30rocblas_internal_gemm_templateIdE15rocblas_status_P15_rocblas_handle18rocblas_operation_S3_iiiPKT_S6_lilS6_lilS6_PS4_lili",
             "_Z33rocblas_internal_gemm_template_64IdE15rocblas_status_P15_rocblas_handle18rocblas_operation_S3_lllPKT_S6_lllS6_lllS6_PS4_llll")
ROCBLAS_DECL(c, hipComplex,
             "_Z30rocblas_internal_gemm_templateI19rocblas_complex_numIfEE15rocblas_status_P15_rocblas_handle18rocblas_operation_S5_iiiPKT_S8_lilS8_lilS8_PS6_lili",
             "_Z33rocblas_internal_gemm_template_64I19rocblas_complex_numIfEE15rocblas_status_P15_rocblas_handle18rocblas_operation_S5_lllPKT_S8_lllS8_lllS8_PS6_llll")
ROCBLAS_DECL(z, hipDoubleComplex,
             "_Z30rocblas_internal_gemm_templateI19rocblas_complex_numIdEE15rocblas_status_P15_rocblas_handle18rocblas_operation_S5_iiiPKT_S8_lilS8_lilS8_PS6_lili",
             "_Z33rocblas_internal_gemm_template_64I19rocblas_complex_numIdEE15rocblas_status_P15_rocblas_handle18rocblas_operation_S5_lllPKT_S8_lllS8_lllS8_PS6_llll")
#undef ROCBLAS_DECL
}
#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

static void one_thread(int id) {
    hipblasHandle_t h;
    mock_create(&h);
    const double one = 1, zero = 0;
    const float onef = 1, zerof = 0;
    std::vector<double> A(600 * 600), B(600 * 600), C(600 * 600);
    std::vector<float> fA(300 * 300), fB(300 * 300), fC(300 * 300);
    const int shapes[][3] = {{64, 48, 100}, {300, 200, 520}, {64, 48, 100}, {600, 600, 257}, {1, 1, 1}, {300, 200, 520}};
    for (int rep = 0; rep < 3; ++rep)
        for (auto& s : shapes) {
            if (rep == 1) mock_set_stream(h, (hipStream_t)(uintptr_t)(0x1000 + id));  // stream switch -> event hand-off
            CHECK(hipblasDgemm(h, HIPBLAS_OP_N, HIPBLAS_OP_T, s[0], s[1], s[2], &one, A.data(), s[0], B.data(), s[1], &zero, C.data(), s[0]) == HIPBLAS_STATUS_SUCCESS);
            CHECK(hipblasDgemm(h, HIPBLAS_OP_N, HIPBLAS_OP_T, s[0], s[1], s[2], &one, A.data(), s[0], B.data(), s[1], &zero, C.data(), s[0]) == HIPBLAS_STATUS_SUCCESS);  // same pointers: skip cache
            CHECK(hipblasSgemm(h, HIPBLAS_OP_T, HIPBLAS_OP_N, 200, 150, 300, &onef, fA.data(), 300, fB.data(), 300, &zerof, fC.data(), 200) == HIPBLAS_STATUS_SUCCESS);
        }
    CHECK(hipblasDgemm_64(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 100, 90, 80, &one, A.data(), 100, B.data(), 80, &zero, C.data(), 100) == HIPBLAS_STATUS_SUCCESS);
    CHECK(hipblasGemmEx(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 100, 90, 80, &one, A.data(), HIP_R_64F, 100, B.data(), HIP_R_64F, 80, &zero, C.data(), HIP_R_64F, 100,
                        HIPBLAS_COMPUTE_64F, HIPBLAS_GEMM_DEFAULT) == HIPBLAS_STATUS_SUCCESS);
    CHECK(hipblasGemmEx(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 100, 90, 80, &one, A.data(), HIP_R_16F, 100, B.data(), HIP_R_16F, 80, &zero, C.data(), HIP_R_16F, 100,
                        HIPBLAS_COMPUTE_32F, HIPBLAS_GEMM_DEFAULT) == HIPBLAS_STATUS_SUCCESS);  // not an emulated type: native
    {  // batched: one set of launches (INT8 backend default), then 7 items over the default 4 lanes (own streams and workspaces,
       // fork / join events), then serial with one lane
        const long emu_a = mock_emulated_calls();
        CHECK(hipblasDgemmStridedBatched(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 50, 40, 30, &one, A.data(), 50, 1500, B.data(), 30, 1200, &zero, C.data(), 50, 2000, 7) ==
              HIPBLAS_STATUS_SUCCESS);
        CHECK(mock_emulated_calls() >= emu_a + 7);
        // the environment is process state and setenv is not thread-safe against getenv: only the first, sequential pass (id 0)
        // switches the batch paths; the concurrent passes run the default one
        if (id != 0) goto batch_done;
        setenv("GEMMUL8_BATCH_WORKSPACE_MB", "1", 1);  // smaller than one item: chunks of a single item, the buffer is re-grown
        const long emu_c = mock_emulated_calls();
        CHECK(hipblasDgemmStridedBatched(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 50, 40, 30, &one, A.data(), 50, 1500, B.data(), 30, 1200, &zero, C.data(), 50, 2000, 5) ==
              HIPBLAS_STATUS_SUCCESS);
        CHECK(mock_emulated_calls() >= emu_c + 5);
        unsetenv("GEMMUL8_BATCH_WORKSPACE_MB");
        setenv("GEMMUL8_BATCH_FUSED", "0", 1);
        const long emu_b = mock_emulated_calls();
        CHECK(hipblasDgemmStridedBatched(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 50, 40, 30, &one, A.data(), 50, 1500, B.data(), 30, 1200, &zero, C.data(), 50, 2000, 7) ==
              HIPBLAS_STATUS_SUCCESS);
        CHECK(mock_emulated_calls() >= emu_b + 7);  // (other threads count too)
        setenv("GEMMUL8_BATCH_STREAMS", "1", 1);
        CHECK(hipblasDgemmStridedBatched(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 50, 40, 30, &one, A.data(), 50, 1500, B.data(), 30, 1200, &zero, C.data(), 50, 2000, 3) ==
              HIPBLAS_STATUS_SUCCESS);
        unsetenv("GEMMUL8_BATCH_STREAMS");
        unsetenv("GEMMUL8_BATCH_FUSED");
    }
batch_done:
    // outside the emulator's range (k > 2^17): native, not an error
    std::vector<double> Ak((size_t)4 * ((1 << 17) + 8)), Bk((size_t)((1 << 17) + 8) * 3);
    const long nat0 = mock_native_calls();
    CHECK(hipblasDgemm(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 4, 3, (1 << 17) + 8, &one, Ak.data(), 4, Bk.data(), (1 << 17) + 8, &zero, C.data(), 4) == HIPBLAS_STATUS_SUCCESS);
    CHECK(mock_native_calls() > nat0);
    // early outs
    CHECK(hipblasDgemm(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 0, 3, 5, &one, A.data(), 1, B.data(), 5, &zero, C.data(), 1) == HIPBLAS_STATUS_SUCCESS);
    CHECK(hipblasDgemm(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 4, 3, 5, &one, nullptr, 4, B.data(), 5, &zero, C.data(), 4) == HIPBLAS_STATUS_INVALID_VALUE);
    // hipblasLt: plain double matmul out of place (emulated), batch 2 (native), bias epilogue (native)
    hipblasLtHandle_t lt = (hipblasLtHandle_t)(uintptr_t)(0x9000 + id);
    void* d = mock_lt_desc(HIPBLAS_OP_T, HIPBLAS_OP_N, HIPBLASLT_EPILOGUE_DEFAULT);
    hipblasLtMatrixLayout_t la, lb, lb2, lc, ld;  // created through the hooked entry points: the hook records what they hold
    CHECK(hipblasLtMatrixLayoutCreate(&la, HIP_R_64F, 80, 100, 80) == HIPBLAS_STATUS_SUCCESS);
    CHECK(hipblasLtMatrixLayoutCreate(&lb, HIP_R_64F, 80, 90, 80) == HIPBLAS_STATUS_SUCCESS);
    CHECK(hipblasLtMatrixLayoutCreate(&lb2, HIP_R_64F, 80, 90, 80) == HIPBLAS_STATUS_SUCCESS);
    CHECK(hipblasLtMatrixLayoutCreate(&lc, HIP_R_64F, 100, 90, 100) == HIPBLAS_STATUS_SUCCESS);
    CHECK(hipblasLtMatrixLayoutCreate(&ld, HIP_R_64F, 100, 90, 104) == HIPBLAS_STATUS_SUCCESS);
    const int32_t two = 2;
    CHECK(hipblasLtMatrixLayoutSetAttribute(lb2, HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT, &two, sizeof two) == HIPBLAS_STATUS_SUCCESS);
    std::vector<double> D(104 * 90);
    const long emu0 = mock_emulated_calls();
    CHECK(hipblasLtMatmul(lt, (hipblasLtMatmulDesc_t)d, &one, A.data(), (hipblasLtMatrixLayout_t)la, B.data(), (hipblasLtMatrixLayout_t)lb, &one, C.data(),
                          (hipblasLtMatrixLayout_t)lc, D.data(), (hipblasLtMatrixLayout_t)ld, nullptr, nullptr, 0, (hipStream_t)(uintptr_t)(0x2000 + id)) == HIPBLAS_STATUS_SUCCESS);
    CHECK(mock_emulated_calls() > emu0);
    const long nat1 = mock_native_calls();
    CHECK(hipblasLtMatmul(lt, (hipblasLtMatmulDesc_t)d, &one, A.data(), (hipblasLtMatrixLayout_t)la, B.data(), (hipblasLtMatrixLayout_t)lb2, &one, C.data(),
                          (hipblasLtMatrixLayout_t)lc, D.data(), (hipblasLtMatrixLayout_t)ld, nullptr, nullptr, 0, nullptr) == HIPBLAS_STATUS_SUCCESS);
    {  // strided batch through hipblasLt (all four layouts with 3 items): emulated as one set of launches
        hipblasLtMatrixLayout_t ba, bb, bc, bd;
        CHECK(hipblasLtMatrixLayoutCreate(&ba, HIP_R_64F, 80, 100, 80) == HIPBLAS_STATUS_SUCCESS);
        CHECK(hipblasLtMatrixLayoutCreate(&bb, HIP_R_64F, 80, 90, 80) == HIPBLAS_STATUS_SUCCESS);
        CHECK(hipblasLtMatrixLayoutCreate(&bc, HIP_R_64F, 100, 90, 100) == HIPBLAS_STATUS_SUCCESS);
        CHECK(hipblasLtMatrixLayoutCreate(&bd, HIP_R_64F, 100, 90, 104) == HIPBLAS_STATUS_SUCCESS);
        const int32_t three = 3;
        const int64_t strides[4] = {8000, 7200, 9000, 9360};
        hipblasLtMatrixLayout_t ls[4] = {ba, bb, bc, bd};
        for (int i = 0; i < 4; ++i) {
            CHECK(hipblasLtMatrixLayoutSetAttribute(ls[i], HIPBLASLT_MATRIX_LAYOUT_BATCH_COUNT, &three, sizeof three) == HIPBLAS_STATUS_SUCCESS);
            CHECK(hipblasLtMatrixLayoutSetAttribute(ls[i], HIPBLASLT_MATRIX_LAYOUT_STRIDED_BATCH_OFFSET, &strides[i], sizeof(int64_t)) == HIPBLAS_STATUS_SUCCESS);
        }
        std::vector<double> D3(3 * 9360);
        const long emu1 = mock_emulated_calls();
        CHECK(hipblasLtMatmul(lt, (hipblasLtMatmulDesc_t)d, &one, A.data(), ba, B.data(), bb, &one, C.data(), bc, D3.data(), bd, nullptr, nullptr, 0,
                              (hipStream_t)(uintptr_t)(0x2000 + id)) == HIPBLAS_STATUS_SUCCESS);
        CHECK(mock_emulated_calls() >= emu1 + 3);
        for (hipblasLtMatrixLayout_t l : ls) CHECK(hipblasLtMatrixLayoutDestroy(l) == HIPBLAS_STATUS_SUCCESS);
    }
    {  // bias epilogue with a bias vector of the matrices' type: emulated GEMM + bias addition
        std::vector<double> bias(100, 0.5);
        void* dbb = mock_lt_desc_bias(HIPBLAS_OP_T, HIPBLAS_OP_N, bias.data(), (int)HIP_R_64F);
        const long emu2 = mock_emulated_calls();
        CHECK(hipblasLtMatmul(lt, (hipblasLtMatmulDesc_t)dbb, &one, A.data(), (hipblasLtMatrixLayout_t)la, B.data(), (hipblasLtMatrixLayout_t)lb, &zero, C.data(),
                              (hipblasLtMatrixLayout_t)lc, D.data(), (hipblasLtMatrixLayout_t)ld, nullptr, nullptr, 0, (hipStream_t)(uintptr_t)(0x2000 + id)) == HIPBLAS_STATUS_SUCCESS);
        CHECK(mock_emulated_calls() > emu2);
        CHECK(((const unsigned char*)D.data())[0] == 0x66);  // the mock's bias pass ran last
        mock_lt_free_desc(dbb);
    }
    void* db = mock_lt_desc(HIPBLAS_OP_T, HIPBLAS_OP_N, HIPBLASLT_EPILOGUE_BIAS);  // no bias pointer: left to the native routine
    CHECK(hipblasLtMatmul(lt, (hipblasLtMatmulDesc_t)db, &one, A.data(), (hipblasLtMatrixLayout_t)la, B.data(), (hipblasLtMatrixLayout_t)lb, &one, C.data(),
                          (hipblasLtMatrixLayout_t)lc, D.data(), (hipblasLtMatrixLayout_t)ld, nullptr, nullptr, 0, nullptr) == HIPBLAS_STATUS_SUCCESS);
    CHECK(mock_native_calls() >= nat1 + 2);
    mock_lt_free_desc(d), mock_lt_free_desc(db);
    for (hipblasLtMatrixLayout_t l : {la, lb, lb2, lc, ld}) CHECK(hipblasLtMatrixLayoutDestroy(l) == HIPBLAS_STATUS_SUCCESS);
    CHECK(hipblasLtDestroy(lt) == HIPBLAS_STATUS_SUCCESS);
    CHECK(hipblasDestroy(h) == HIPBLAS_STATUS_SUCCESS);  // frees the handle's three buffers first
}

// Every exported GEMM entry point once where the environment selects its type (emulated: the emulation's counter rises, the native one
// does not) and once where it does not -- the type's GEMMUL8_NUM_MOD_* unset, or GEMMUL8_HOOK_ROCBLAS unset for the rocBLAS names -- where
// exactly one native call is made.  Single-threaded: it switches the environment between calls.
template <typename F> static void emulated_then_native(F call, bool rocblas) {
    const char* const nmod[4][2] = {{"GEMMUL8_NUM_MOD_S", "8"}, {"GEMMUL8_NUM_MOD_D", "15"}, {"GEMMUL8_NUM_MOD_C", "8"}, {"GEMMUL8_NUM_MOD_Z", "15"}};
    for (auto& v : nmod) setenv(v[0], v[1], 1);
    if (rocblas) setenv("GEMMUL8_HOOK_ROCBLAS", "1", 1);
    long emu = mock_emulated_calls(), nat = mock_native_calls();
    CHECK(call() == 0);  // HIPBLAS_STATUS_SUCCESS == rocblas_status_success == 0
    CHECK(mock_emulated_calls() > emu);
    CHECK(mock_native_calls() == nat);
    if (rocblas) unsetenv("GEMMUL8_HOOK_ROCBLAS");
    else
        for (auto& v : nmod) unsetenv(v[0]);
    emu = mock_emulated_calls(), nat = mock_native_calls();
    CHECK(call() == 0);
    CHECK(mock_emulated_calls() == emu);
    CHECK(mock_native_calls() == nat + 1);
    for (auto& v : nmod) unsetenv(v[0]);
}
template <typename T, typename Gemm, typename Gemm64, typename Sb, typename RGemm, typename RSb, typename RInt32, typename RInt64>
static void every_typed_entry_point(hipblasHandle_t h, hipDataType type, hipblasComputeType_t compute, int rocblas_type, Gemm gemm, Gemm64 gemm_64, Sb sb,
                                    RGemm rgemm, RSb rsb, RInt32 rint32, RInt64 rint64) {
    const int m = 40, n = 30, k = 20, batch = 3;
    const long long sa = m * k, sb_ = k * n, sc = m * n;
    std::vector<T> A(sa * batch), B(sb_ * batch), C(sc * batch);
    const T one{1}, zero{0};
    const hipblasOperation_t N = HIPBLAS_OP_N;
    emulated_then_native([&] { return (int)gemm(h, N, N, m, n, k, &one, A.data(), m, B.data(), k, &zero, C.data(), m); }, false);
    emulated_then_native([&] { return (int)gemm_64(h, N, N, m, n, k, &one, A.data(), m, B.data(), k, &zero, C.data(), m); }, false);
    emulated_then_native([&] { return (int)hipblasGemmEx(h, N, N, m, n, k, &one, A.data(), type, m, B.data(), type, k, &zero, C.data(), type, m, compute, HIPBLAS_GEMM_DEFAULT); }, false);
    emulated_then_native([&] { return (int)hipblasGemmEx_64(h, N, N, m, n, k, &one, A.data(), type, m, B.data(), type, k, &zero, C.data(), type, m, compute, HIPBLAS_GEMM_DEFAULT); }, false);
    emulated_then_native([&] { return (int)hipblasGemmExWithFlags(h, N, N, m, n, k, &one, A.data(), type, m, B.data(), type, k, &zero, C.data(), type, m, compute, HIPBLAS_GEMM_DEFAULT, HIPBLAS_GEMM_FLAGS_NONE); }, false);
    emulated_then_native([&] { return (int)hipblasGemmExWithFlags_64(h, N, N, m, n, k, &one, A.data(), type, m, B.data(), type, k, &zero, C.data(), type, m, compute, HIPBLAS_GEMM_DEFAULT, HIPBLAS_GEMM_FLAGS_NONE); }, false);
    emulated_then_native([&] { return (int)sb(h, N, N, m, n, k, &one, A.data(), m, sa, B.data(), k, sb_, &zero, C.data(), m, sc, batch); }, false);
    emulated_then_native([&] { return (int)hipblasGemmStridedBatchedEx(h, N, N, m, n, k, &one, A.data(), type, m, sa, B.data(), type, k, sb_, &zero, C.data(), type, m, sc, batch, compute, HIPBLAS_GEMM_DEFAULT); }, false);
    // rocBLAS: 111 = rocblas_operation_none; the handle of a hipBLAS call is the rocBLAS handle
    emulated_then_native([&] { return rgemm(h, 111, 111, m, n, k, &one, A.data(), m, B.data(), k, &zero, C.data(), m); }, true);
    emulated_then_native([&] { return rsb(h, 111, 111, m, n, k, &one, A.data(), m, sa, B.data(), k, sb_, &zero, C.data(), m, sc, batch); }, true);
    emulated_then_native([&] { return rocblas_gemm_ex(h, 111, 111, m, n, k, &one, A.data(), rocblas_type, m, B.data(), rocblas_type, k, &zero, C.data(), rocblas_type, m, C.data(), rocblas_type, m, rocblas_type, 0, 0, 0); }, true);
    emulated_then_native([&] { return rint32(h, 111, 111, m, n, k, &one, A.data(), 0, m, sa, B.data(), 0, k, sb_, &zero, C.data(), 0, m, sc, 1); }, true);  // one item
    emulated_then_native([&] { return rint64(h, 111, 111, m, n, k, &one, A.data(), 0, m, sa, B.data(), 0, k, sb_, &zero, C.data(), 0, m, sc, batch); }, true);  // strided batch
}
static void every_entry_point() {
    hipblasHandle_t h;
    mock_create(&h);
    every_typed_entry_point<float>(h, HIP_R_32F, HIPBLAS_COMPUTE_32F, 151, hipblasSgemm, hipblasSgemm_64, hipblasSgemmStridedBatched, rocblas_sgemm,
                                   rocblas_sgemm_strided_batched, rb_int_s_32, rb_int_s_64);
    every_typed_entry_point<double>(h, HIP_R_64F, HIPBLAS_COMPUTE_64F, 152, hipblasDgemm, hipblasDgemm_64, hipblasDgemmStridedBatched, rocblas_dgemm,
                                    rocblas_dgemm_strided_batched, rb_int_d_32, rb_int_d_64);
    every_typed_entry_point<hipComplex>(h, HIP_C_32F, HIPBLAS_COMPUTE_32F, 154, hipblasCgemm, hipblasCgemm_64, hipblasCgemmStridedBatched, rocblas_cgemm,
                                        rocblas_cgemm_strided_batched, rb_int_c_32, rb_int_c_64);
    every_typed_entry_point<hipDoubleComplex>(h, HIP_C_64F, HIPBLAS_COMPUTE_64F, 155, hipblasZgemm, hipblasZgemm_64, hipblasZgemmStridedBatched, rocblas_zgemm,
                                              rocblas_zgemm_strided_batched, rb_int_z_32, rb_int_z_64);
    setenv("GEMMUL8_NUM_MOD_D", "15", 1);
    const double one = 1, zero = 0;
    std::vector<double> A(40 * 20 * 3), B(20 * 30 * 3), C(40 * 30 * 3);
    const hipblasOperation_t N = HIPBLAS_OP_N;
    // an ILP64 form with a dimension an int cannot hold: native (the stand-in reads no operand)
    long nat = mock_native_calls(), emu = mock_emulated_calls();
    CHECK(hipblasDgemm_64(h, N, N, 40, 30, 20, &one, A.data(), (int64_t)2147483647 + 41, B.data(), 20, &zero, C.data(), 40) == HIPBLAS_STATUS_SUCCESS);
    CHECK(mock_native_calls() == nat + 1 && mock_emulated_calls() == emu);
    // the ILP64 forms keep the plain forms' early outs
    CHECK(hipblasDgemm_64(h, N, N, 40, 0, 20, &one, A.data(), 40, B.data(), 20, &zero, C.data(), 40) == HIPBLAS_STATUS_SUCCESS);
    CHECK(hipblasGemmExWithFlags_64(h, N, N, 40, 30, 20, &one, A.data(), HIP_R_64F, 40, nullptr, HIP_R_64F, 20, &zero, C.data(), HIP_R_64F, 40, HIPBLAS_COMPUTE_64F,
                                    HIPBLAS_GEMM_DEFAULT, HIPBLAS_GEMM_FLAGS_NONE) == HIPBLAS_STATUS_INVALID_VALUE);
    CHECK(mock_native_calls() == nat + 1 && mock_emulated_calls() == emu);
    // the strided-batched forms do NOT early-out: an empty batch is the native routine's to answer
    CHECK(hipblasDgemmStridedBatched(h, N, N, 40, 30, 20, &one, A.data(), 40, 800, B.data(), 20, 600, &zero, C.data(), 40, 1200, 0) == HIPBLAS_STATUS_SUCCESS);
    CHECK(mock_native_calls() == nat + 2 && mock_emulated_calls() == emu);
    CHECK(hipblasGemmStridedBatchedEx(h, N, N, 40, 30, 20, &one, A.data(), HIP_R_64F, 40, 800, B.data(), HIP_R_64F, 20, 600, &zero, C.data(), HIP_R_64F, 40, 1200, 0,
                                      HIPBLAS_COMPUTE_64F, HIPBLAS_GEMM_DEFAULT) == HIPBLAS_STATUS_SUCCESS);
    CHECK(mock_native_calls() == nat + 3 && mock_emulated_calls() == emu);
    // rocblas_gemm_ex serves only the in-place form: c != d is rocBLAS's
    setenv("GEMMUL8_HOOK_ROCBLAS", "1", 1);
    CHECK(rocblas_gemm_ex(h, 111, 111, 40, 30, 20, &one, A.data(), 152, 40, B.data(), 152, 20, &zero, C.data(), 152, 40, C.data() + 1200, 152, 40, 152, 0, 0, 0) == 0);
    CHECK(mock_native_calls() == nat + 4 && mock_emulated_calls() == emu);
    unsetenv("GEMMUL8_HOOK_ROCBLAS");
    CHECK(rocblas_destroy_handle(h) == 0);  // releases the state the rocBLAS calls left under this handle, then the handle
    setenv("GEMMUL8_NUM_MOD_S", "8", 1);
}

int main() {
    setenv("GEMMUL8_HOOK_STATS", "1", 1);  // the line printed at exit counts every call above and below
    setenv("GEMMUL8_NUM_MOD_D", "15", 1);
    setenv("GEMMUL8_NUM_MOD_S", "8", 1);
    setenv("GEMMUL8_SKIP_SCALE_A", "1", 1);
    setenv("GEMMUL8_SKIP_SCALE_B", "1", 1);
    setenv("GEMMUL8_MAX_M", "256", 1);
    setenv("GEMMUL8_MAX_N", "256", 1);
    setenv("GEMMUL8_MAX_K", "512", 1);
    setenv("GEMMUL8_MAX_NUM_MOD", "15", 1);
    one_thread(0);
    every_entry_point();
    std::vector<std::thread> ts;
    for (int i = 1; i <= 4; ++i) ts.emplace_back(one_thread, i);
    for (auto& t : ts) t.join();
    // the size floor and the environment switch are read on every call
    hipblasHandle_t h;
    mock_create(&h);
    const double one = 1, zero = 0;
    std::vector<double> A(64 * 64), B(64 * 64), C(64 * 64);
    setenv("GEMMUL8_MIN_FLOPS", "1000000000", 1);
    long nat = mock_native_calls();
    CHECK(hipblasDgemm(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 64, 64, 64, &one, A.data(), 64, B.data(), 64, &zero, C.data(), 64) == HIPBLAS_STATUS_SUCCESS);
    CHECK(mock_native_calls() == nat + 1);
    setenv("GEMMUL8_MIN_FLOPS", "auto", 1);  // the opt-in fitted cost model: a 64^3 call is far below the measured crossover -> native again
    nat = mock_native_calls();
    CHECK(hipblasDgemm(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 64, 64, 64, &one, A.data(), 64, B.data(), 64, &zero, C.data(), 64) == HIPBLAS_STATUS_SUCCESS);
    CHECK(mock_native_calls() == nat + 1);
    unsetenv("GEMMUL8_MIN_FLOPS");  // unset = emulate every selected call (the reference's behaviour)
    {
        const long emu0 = mock_emulated_calls();
        CHECK(hipblasDgemm(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 64, 64, 64, &one, A.data(), 64, B.data(), 64, &zero, C.data(), 64) == HIPBLAS_STATUS_SUCCESS);
        CHECK(mock_emulated_calls() == emu0 + 1);
    }
    setenv("GEMMUL8_DIST", "blocks", 1);  // no RANK / WORLD_SIZE: one warning, then single-GPU emulation
    long emu = mock_emulated_calls();
    CHECK(hipblasDgemm(h, HIPBLAS_OP_N, HIPBLAS_OP_N, 64, 64, 64, &one, A.data(), 64, B.data(), 64, &zero, C.data(), 64) == HIPBLAS_STATUS_SUCCESS);
    CHECK(mock_emulated_calls() == emu + 1);
    CHECK(hipblasDestroy(h) == HIPBLAS_STATUS_SUCCESS);
    CHECK(mock_live_allocs() == 0);  // every workspace of every destroyed handle was released
    std::printf("hook under sanitizers: %ld emulated, %ld native calls ALL OK\n", mock_emulated_calls(), mock_native_calls());
    return 0;
}
