// Leaf solve of gemmul8_trsm (include/gemmul8_c.h): one diagonal block of M = op(Atri) of order r <= L against the right-hand sides of B, in place.
// No counterpart in the reference (it emulates GEMM only).
//
// The canonical problem.  Whatever side, triangle and op, the block is brought to ONE form while it is staged: a LOWER triangle c(p, q), q <= p, and
// right-hand-side vectors b(p), solved forwards --
//     for p = 0 .. r-1:  acc = s (x) b(p);  for q = 0 .. p-1 ascending: acc = acc (-) (c(p, q) (x) x(q));  x(p) = acc  or  acc (/) c(p, p)
// with    LEFT,  M lower:  c(p, q) = M(p, q),              b(p) = row p of B
//         LEFT,  M upper:  c(p, q) = M(r-1-p, r-1-q),      b(p) = row r-1-p          (i descending, j descending from r-1 to i+1)
//         RIGHT, M upper:  c(p, q) = M(q, p),              b(p) = column p           (j and i ascending)
//         RIGHT, M lower:  c(p, q) = M(r-1-q, r-1-p),      b(p) = column r-1-p       (both descending)
// which is the header's order of operations for each of the four (the real product commutes bit for bit, and so does the textbook complex one: its
// real part is the same expression and its imaginary part the same two products under a commutative sum).
//
// Column-oriented: once x(q) is final, every later row takes its update independently.  A workgroup holds W right-hand sides; thread (c, g) owns the rows
// p = g + G k, k < 16, of right-hand side c in registers.  Step q: the owner of row q divides and publishes x(q) of its W right-hand sides in LDS
// (double-buffered: one barrier per step), then every thread updates its rows below q -- 16 - q / G independent chains per thread.  g is wave-uniform
// (W = 64), so the owner test and the first partial row are uniform branches, and c(p, q) is one LDS address per wave (a broadcast read).
//
// The triangle is staged ONCE per workgroup, packed (c(p, q) at p (p + 1) / 2 + q), by the address rule of the triangular form of oz2_scale.hip (sym_at):
// memory element (f, s) of the stored array is read where the stored triangle holds it, the dead half is never addressed and a unit diagonal is a 1 without
// a load; the walk is f-fastest, so the loads are coalesced.  Right-hand sides: RIGHT -- lane c is a row of B, contiguous for every p; LEFT -- the
// r x W tile goes through LDS, read and written p-fastest (a column of B) and handed to the threads transposed.
//
// Rounding: every (x), (-), (/) is one IEEE operation of the element type.  The file is built with -ffp-contract=off like the rest of the library and
// repeats it below; `/` is the correctly rounded division (hipcc's default for FP32 as well as FP64).
#include <hip/hip_runtime.h>
#include <string.h>

#include <atomic>

#include "oz2_kernels.h"

#pragma clang fp contract(off)

namespace oz2 {

#ifndef OZ2_TRSM_LEAF
// 64 or 128.  profiles/trsm_ab.json (tools/trsm_ab.py, both builds interleaved): DTRSM 8192 x 8192 25.1 ms at 64 against 19.6 ms at 128, ZTRSM 4096 x 4096
// 15.5 ms against 21.0 ms (at 128 a complex128 strip is 8 right-hand sides wide: the triangle takes 132 of the 160 KiB).  The two relative differences are
// alike with opposite signs; 64 is kept: the order the GPU suite was run with.
#define OZ2_TRSM_LEAF 64
#endif
static_assert(OZ2_TRSM_LEAF == 64 || OZ2_TRSM_LEAF == 128, "the leaf order is 64 or 128");
int trsm_leaf_order() { return OZ2_TRSM_LEAF; }

namespace {

constexpr int kLeaf = OZ2_TRSM_LEAF;
constexpr int kRpt = 16;  // rows of a right-hand side per thread

// a complex element as a plain aggregate (the layout of cfloat / cdouble): the per-thread rows stay in registers
template <typename R> struct alignas(2 * sizeof(R)) Cplx {
    R x, y;
};
using cfloat = Cplx<float>;
using cdouble = Cplx<double>;
template <typename T> struct Elem {
    static constexpr bool cplx = false;
    using real = T;
};
template <typename R> struct Elem<Cplx<R>> {
    static constexpr bool cplx = true;
    using real = R;
};

template <typename T> __device__ __forceinline__ T e_zero() {
    if constexpr (Elem<T>::cplx) return T{0, 0};
    else return T(0);
}
template <typename T> __device__ __forceinline__ T e_one() {
    if constexpr (Elem<T>::cplx) return T{1, 0};
    else return T(1);
}
// the textbook product: four products, two sums
template <typename T> __device__ __forceinline__ T e_mul(T a, T b) {
    if constexpr (Elem<T>::cplx) {
        T r;
        r.x = a.x * b.x - a.y * b.y;
        r.y = a.x * b.y + a.y * b.x;
        return r;
    } else {
        return a * b;
    }
}
template <typename T> __device__ __forceinline__ T e_sub(T a, T b) {
    if constexpr (Elem<T>::cplx) return T{a.x - b.x, a.y - b.y};
    else return a - b;
}
// the textbook quotient, NOT scaled against overflow of den
template <typename T> __device__ __forceinline__ T e_div(T a, T d) {
    if constexpr (Elem<T>::cplx) {
        const auto den = d.x * d.x + d.y * d.y;
        T r;
        r.x = (a.x * d.x + a.y * d.y) / den;
        r.y = (a.y * d.x - a.x * d.y) / den;
        return r;
    } else {
        return a / d;
    }
}

struct LeafArgs {
    const void* A;  // element (0, 0) of the diagonal block in the stored array
    size_t lda;
    void* B;  // LEFT: first row of the block's rows of B; RIGHT: first column
    size_t ldb;
    const void* alpha_dev;  // scaled: the device-resident alpha, or nullptr = alpha_host
    alignas(16) unsigned char alpha_host[16];
    unsigned r, nrhs;
    int left, lower_a, swap, rev, conj, unit;
};

// strip width: 64 right-hand sides (one per lane); complex128 at L = 128 has 28 KiB left beside its 132 KiB triangle
template <typename T> constexpr int strip_of() { return (kLeaf == 128 && sizeof(T) == 16) ? 8 : 64; }
template <typename T> constexpr size_t leaf_lds_bytes() {
    return sizeof(T) * ((size_t)kLeaf * (kLeaf + 1) / 2 + 2 * strip_of<T>() + (size_t)strip_of<T>() * (kLeaf + 1));
}

template <typename T, bool SCALED> __global__ __launch_bounds__(strip_of<T>() * (kLeaf / kRpt)) void trsm_leaf_kernel(const LeafArgs a) {
    constexpr int L = kLeaf, W = strip_of<T>(), G = L / kRpt, NT = W * G, LDT = L + 1;
    extern __shared__ __attribute__((aligned(16))) char trsm_lds[];
    T* const tri = reinterpret_cast<T*>(trsm_lds);  // packed lower triangle, L (L + 1) / 2
    T* const xs = tri + L * (L + 1) / 2;            // x(q) of the W right-hand sides, two buffers
    T* const tile = xs + 2 * W;                     // LEFT: the r x W tile, right-hand side c at c * LDT
    const unsigned t = threadIdx.x, c = t % W, g = t / W, r = a.r;
    const size_t rhs0 = (size_t)blockIdx.x * W;
    const unsigned nc = a.nrhs - rhs0 < (size_t)W ? (unsigned)(a.nrhs - rhs0) : (unsigned)W;
    const bool unit = a.unit != 0, rev = a.rev != 0;

    // ---- the triangle, once per workgroup
    {
        const T* const A = static_cast<const T*>(a.A);
        for (unsigned e = t; e < (unsigned)(L * L); e += NT) {
            const unsigned f = e % L, s = e / L;  // memory element (row f, column s)
            if (f >= r || s >= r) continue;
            if (a.lower_a ? f < s : f > s) continue;  // the other strict triangle: never addressed
            T v;
            if (f == s && unit) {
                v = e_one<T>();  // (never used by the solve: kept so that every staged entry is defined)
            } else {
                v = A[(size_t)s * a.lda + f];
                if constexpr (Elem<T>::cplx)
                    if (a.conj) v.y = -v.y;
            }
            unsigned p = a.swap ? s : f, q = a.swap ? f : s;
            if (rev) p = r - 1 - p, q = r - 1 - q;
            tri[p * (p + 1) / 2 + q] = v;
        }
    }
    // ---- the right-hand sides
    T* const B = static_cast<T*>(a.B);
    // a thread's rows, components apart (an array of aggregates does not leave scratch memory)
    typename Elem<T>::real accx[kRpt], accy[Elem<T>::cplx ? kRpt : 1];
    auto get = [&](int k) -> T {
        if constexpr (Elem<T>::cplx) return T{accx[k], accy[k]};
        else return accx[k];
    };
    auto put = [&](int k, T v) {
        if constexpr (Elem<T>::cplx) accx[k] = v.x, accy[k] = v.y;
        else accx[k] = v;
    };
    if (a.left) {
        for (unsigned e = t; e < (unsigned)(L * W); e += NT) {
            const unsigned pm = e % L, cc = e / L;
            if (pm < r && cc < nc) tile[cc * LDT + pm] = B[(rhs0 + cc) * a.ldb + pm];
        }
    }
    __syncthreads();
    T s = e_one<T>();
    if constexpr (SCALED) s = a.alpha_dev ? *static_cast<const T*>(a.alpha_dev) : *reinterpret_cast<const T*>(a.alpha_host);
#pragma unroll
    for (int k = 0; k < kRpt; ++k) {
        const unsigned p = k * G + g;
        T v = e_zero<T>();
        if (p < r && c < nc) {
            const unsigned pm = rev ? r - 1 - p : p;
            v = a.left ? tile[c * LDT + pm] : B[(size_t)pm * a.ldb + rhs0 + c];
            if constexpr (SCALED) v = e_mul(s, v);
        }
        put(k, v);
    }
    // ---- the solve
#pragma unroll
    for (int kk = 0; kk < kRpt; ++kk) {
        if ((unsigned)(kk * G) >= r) break;
        for (int jj = 0; jj < G; ++jj) {
            const unsigned q = kk * G + jj;
            if (q >= r) break;
            T* const xq = xs + (q & 1) * W;
            if (g == (unsigned)jj) {
                if (!unit) put(kk, e_div(get(kk), tri[q * (q + 1) / 2 + q]));
                xq[c] = get(kk);
            }
            __syncthreads();
            const T x = xq[c];
            if (g > (unsigned)jj) {
                const unsigned p = kk * G + g;
                if (p < r) put(kk, e_sub(get(kk), e_mul(tri[p * (p + 1) / 2 + q], x)));
            }
#pragma unroll
            for (int k = kk + 1; k < kRpt; ++k) {
                const unsigned p = k * G + g;
                if (p < r) put(k, e_sub(get(k), e_mul(tri[p * (p + 1) / 2 + q], x)));
            }
        }
    }
    // ---- X over B
    if (a.left) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kRpt; ++k) {
            const unsigned p = k * G + g;
            if (p < r && c < nc) tile[c * LDT + (rev ? r - 1 - p : p)] = get(k);
        }
        __syncthreads();
        for (unsigned e = t; e < (unsigned)(L * W); e += NT) {
            const unsigned pm = e % L, cc = e / L;
            if (pm < r && cc < nc) B[(rhs0 + cc) * a.ldb + pm] = tile[cc * LDT + pm];
        }
    } else {
#pragma unroll
        for (int k = 0; k < kRpt; ++k) {
            const unsigned p = k * G + g;
            if (p < r && c < nc) B[(size_t)(rev ? r - 1 - p : p) * a.ldb + rhs0 + c] = get(k);
        }
    }
}

template <typename T, bool SCALED> hipError_t launch_leaf(hipStream_t stream, const LeafArgs& a) {
    constexpr size_t lds = leaf_lds_bytes<T>();
    static_assert(lds <= 160 * 1024, "the leaf's LDS must fit a CU");
    if constexpr (lds > 48 * 1024) {  // (the attribute belongs to the function on one device; setting it is idempotent: oz2_gemm_f8.hip)
        static std::atomic<bool> attr_set_dev[64];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
        if (!attr_set_dev[dev].load(std::memory_order_acquire)) {
            hipError_t e = hipFuncSetAttribute((const void*)trsm_leaf_kernel<T, SCALED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            attr_set_dev[dev].store(true, std::memory_order_release);
        }
    }
    constexpr int W = strip_of<T>();
    const size_t groups = ((size_t)a.nrhs + W - 1) / W;
    hipLaunchKernelGGL((trsm_leaf_kernel<T, SCALED>), dim3((unsigned)groups), dim3(W * (kLeaf / kRpt)), lds, stream, a);
    return hipGetLastError();
}

// the GEMMs' constants for a device-resident alpha: -1 at p, +1 at p + 16 bytes, in the element type
template <typename T> __global__ void trsm_consts_kernel(T* p) {
    if (threadIdx.x == 0) {
        T one = e_one<T>(), minus = e_zero<T>();
        if constexpr (Elem<T>::cplx) minus.x = -1;
        else minus = T(-1);
        p[0] = minus;
        p[16 / sizeof(T)] = one;
    }
}

template <typename T> __global__ void trsm_zero_fill_kernel(T* B, size_t ldb, size_t m, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y;
    if (i < m && j < n) B[j * ldb + i] = e_zero<T>();
}

}  // namespace

hipError_t launch_trsm_leaf(hipStream_t stream, int dtype, bool left, bool lower_a, int transA, bool unit, unsigned r, size_t nrhs, const void* A, size_t lda,
                            void* B, size_t ldb, bool scaled, const void* alpha, bool alpha_on_device) {
    if (r == 0 || nrhs == 0) return hipSuccess;
    if (r > (unsigned)kLeaf || nrhs > 0xFFFFFFFFull) return hipErrorInvalidValue;
    LeafArgs a{};
    a.A = A, a.lda = lda, a.B = B, a.ldb = ldb;
    a.r = r, a.nrhs = (unsigned)nrhs;
    a.left = left, a.lower_a = lower_a, a.unit = unit;
    const bool lower_m = lower_a == (transA == 0);
    a.swap = (transA != 0) != !left;  // canonical (p, q) from memory (f, s): through op, and through the transposition of the RIGHT problem
    a.rev = left ? !lower_m : lower_m;
    a.conj = transA == 2;
    if (scaled) {
        if (alpha_on_device) a.alpha_dev = alpha;
        else memcpy(a.alpha_host, alpha, (is_f32(dtype) ? 4 : 8) * (is_complex(dtype) ? 2 : 1));
    }
    switch (dtype * 2 + (scaled ? 1 : 0)) {
        case 0: return launch_leaf<float, false>(stream, a);
        case 1: return launch_leaf<float, true>(stream, a);
        case 2: return launch_leaf<double, false>(stream, a);
        case 3: return launch_leaf<double, true>(stream, a);
        case 4: return launch_leaf<cfloat, false>(stream, a);
        case 5: return launch_leaf<cfloat, true>(stream, a);
        case 6: return launch_leaf<cdouble, false>(stream, a);
        case 7: return launch_leaf<cdouble, true>(stream, a);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_trsm_consts(hipStream_t stream, int dtype, void* tail) {
    switch (dtype) {
        case kF32: hipLaunchKernelGGL(trsm_consts_kernel<float>, dim3(1), dim3(64), 0, stream, (float*)tail); break;
        case kF64: hipLaunchKernelGGL(trsm_consts_kernel<double>, dim3(1), dim3(64), 0, stream, (double*)tail); break;
        case kC32: hipLaunchKernelGGL(trsm_consts_kernel<cfloat>, dim3(1), dim3(64), 0, stream, (cfloat*)tail); break;
        case kC64: hipLaunchKernelGGL(trsm_consts_kernel<cdouble>, dim3(1), dim3(64), 0, stream, (cdouble*)tail); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_trsm_zero_fill(hipStream_t stream, int dtype, size_t m, size_t n, void* B, size_t ldb) {
    if (m == 0 || n == 0) return hipSuccess;
    const dim3 block(256);
    for (size_t j0 = 0; j0 < n; j0 += 65535) {  // gridDim.y limit
        const size_t nj = n - j0 < 65535 ? n - j0 : 65535;
        const dim3 grid((unsigned)((m + 255) / 256), (unsigned)nj);
        const size_t esz = (is_f32(dtype) ? 4 : 8) * (is_complex(dtype) ? 2 : 1);
        void* Bj = (char*)B + j0 * ldb * esz;
        switch (dtype) {
            case kF32: hipLaunchKernelGGL(trsm_zero_fill_kernel<float>, grid, block, 0, stream, (float*)Bj, ldb, m, nj); break;
            case kF64: hipLaunchKernelGGL(trsm_zero_fill_kernel<double>, grid, block, 0, stream, (double*)Bj, ldb, m, nj); break;
            case kC32: hipLaunchKernelGGL(trsm_zero_fill_kernel<cfloat>, grid, block, 0, stream, (cfloat*)Bj, ldb, m, nj); break;
            case kC64: hipLaunchKernelGGL(trsm_zero_fill_kernel<cdouble>, grid, block, 0, stream, (cdouble*)Bj, ldb, m, nj); break;
            default: return hipErrorInvalidValue;
        }
    }
    return hipGetLastError();
}

}  // namespace oz2
