"""Helpers for the -m gpu parity tests: run the HIP path through the C ABI and fetch intermediates."""
import ctypes as C

import numpy as np
import torch

import gemmul8_amd as g
import oracle_lib as ol

NP2T = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64,
        np.dtype(np.complex64): torch.complex64, np.dtype(np.complex128): torch.complex128}


SAFE, REFERENCE = ol.FP8_BOUND_SAFE, ol.FP8_BOUND_REFERENCE


def select_fp8_bound_mode(mode):
    """Select the FP8 accurate-mode bound inflation on BOTH sides: the product (gemmul8_set_fp8_bound_mode) and the oracle.  SAFE = the
    product's default (engine-safe), REFERENCE = the oracle's default, (k+1)*2^-24 of src/find_max.hpp:82-96."""
    assert g.lib().gemmul8_set_fp8_bound_mode(int(mode)) >= 0
    ol.set_fp8_bound_mode(int(mode))


def restore_fp8_bound_defaults():
    g.lib().gemmul8_set_fp8_bound_mode(SAFE)
    ol.set_fp8_bound_mode(REFERENCE)


def setknob(monkeypatch, name, value):
    """Set (value=None: unset) one of the library's testing knobs for the rest of the test.  The library parses its knobs once
    (csrc/oz2_knobs.hpp), so the environment change is followed by gemmul8_reload_knobs; tests/conftest.py reloads again after the
    test, when monkeypatch has restored the environment."""
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, str(value))
    g.lib().gemmul8_reload_knobs()


def to_dev(M):
    """numpy (rows x cols) matrix -> column-major device tensor of shape (cols, rows)."""
    return torch.from_numpy(np.ascontiguousarray(M.T)).cuda()


def from_dev(T):
    return T.cpu().numpy().T


def f6_plane_values(buf, rows, rows_img, kp):
    """Integer values [rows, kp] of one FP6 panel-image plane of the FP8 backend (gemmul8_layout.lo_format == 1; layout in
    csrc/oz2_gemm_f6.hip): row blocks of 256 (the last one holds rows_img - 256 * nb rows rounded up to 16), K-steps of 128 elements,
    panel = X region (16-byte slot q * Rp + r) + Y region (8-byte slot (q >> 1) * 2 Rp + 2 r + (q & 1)); a fragment packs 32 codes
    sign << 5 | |v| of 6 bits, little-endian."""
    out = np.zeros((rows, kp), np.int8)
    kt_n = kp // 128
    nb = (rows_img + 255) // 256
    blockbytes = 256 * (kp // 4 * 3)
    for tb in range(nb):
        nr = min(256, rows_img - 256 * tb)
        rp = 256 if tb < nb - 1 else (nr + 15) // 16 * 16
        for kt in range(kt_n):
            off = tb * blockbytes + kt * rp * 96
            panel = buf[off:off + rp * 96]
            X = panel[:64 * rp].reshape(4, rp, 16)
            Y = panel[64 * rp:].reshape(2, rp, 2, 8)
            frag = np.concatenate([X, np.stack([Y[0, :, 0], Y[0, :, 1], Y[1, :, 0], Y[1, :, 1]])], axis=2)  # [q][r][24]
            # four 6-bit codes per three bytes, little-endian bit order (c0 = b0[5:0], c1 = b1[3:0] b0[7:6], c2 = b2[1:0] b1[7:4], c3 = b2[7:2])
            b = frag.reshape(4, rp, 8, 3).astype(np.uint16)
            codes = np.stack([b[..., 0] & 63, (b[..., 0] >> 6 | b[..., 1] << 2) & 63, (b[..., 1] >> 4 | b[..., 2] << 4) & 63, b[..., 2] >> 2], axis=3).reshape(4, rp, 32).astype(np.int16)
            vals = np.where(codes & 32, -(codes & 31), codes & 31).astype(np.int8)  # [q][r][32]
            vals = vals.transpose(1, 0, 2).reshape(rp, 128)
            r0, r1 = 256 * tb, min(rows, 256 * tb + rp)
            if r1 > r0:
                out[r0:r1, 128 * kt:128 * kt + 128] = vals[:r1 - r0]
    return out


def f6_plane_image(vals, rows_img, kp, nbytes):
    """Inverse of f6_plane_values: the FP6 panel-image bytes (length nbytes) of integers vals[rows, kp], |v| <= 16; rows beyond vals are zero."""
    buf = np.zeros(nbytes, np.uint8)
    rows = vals.shape[0]
    kt_n = kp // 128
    nb = (rows_img + 255) // 256
    blockbytes = 256 * (kp // 4 * 3)
    for tb in range(nb):
        nr = min(256, rows_img - 256 * tb)
        rp = 256 if tb < nb - 1 else (nr + 15) // 16 * 16
        blk = np.zeros((rp, kp), np.int16)
        r0, r1 = 256 * tb, min(rows, 256 * tb + rp)
        if r1 > r0:
            blk[:r1 - r0] = vals[r0:r1]
        codes = (np.where(blk < 0, 32, 0) | np.abs(blk)).astype(np.uint8)                       # [rp][kp]
        bits = ((codes[..., None] >> np.arange(6, dtype=np.uint8)) & 1).astype(np.uint8)          # [rp][kp][6]
        frag = np.packbits(bits.reshape(rp, kt_n, 4, 32 * 6), axis=3, bitorder="little")          # [rp][kt][q][24]
        for kt in range(kt_n):
            f = frag[:, kt].transpose(1, 0, 2)                                                    # [q][rp][24]
            X = f[:, :, :16]                                                                      # 16-byte slot q * rp + r
            Y = np.zeros((2, rp, 2, 8), np.uint8)                                                 # 8-byte slot (q >> 1) * 2 rp + 2 r + (q & 1)
            for q in range(4):
                Y[q >> 1, :, q & 1] = f[q, :, 16:]
            off = tb * blockbytes + kt * rp * 96
            buf[off:off + 64 * rp] = X.ravel()
            buf[off + 64 * rp:off + 96 * rp] = Y.ravel()
    return buf


def e4m3_of_ints(v):
    """e4m3 byte (OCP, +0 for zero) of integers |v| <= 16: what the reference's planes hold (mod.hpp:159-189)."""
    a = np.abs(v.astype(np.int32))
    e = np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int32), 0)
    mant = np.where(a > 0, (a * 8) // (1 << e) - 8, 0)
    byte = np.where(a > 0, ((e + 7) << 3) | mant, 0) | np.where((v < 0) & (a > 0), 0x80, 0)
    return byte.astype(np.uint8)


def read_intermediates(work, code, backend, m, n, k, N):
    """Shifts, operand planes (decoded to one byte per element) and C_mid of a finished call, read from its workspace through gemmul8_get_layout."""
    cplx = code >= 2
    L = g.Layout()
    g.check(g.lib().gemmul8_get_layout(code, backend, m, n, k, N, work.data_ptr(), None, None, 0, 0, C.byref(L)))
    w = work.cpu().numpy()
    base = work.data_ptr()
    parts, nm = L.parts, L.num_mat

    def region(ptr, nbytes):
        off = ptr - base
        return w[off:off + nbytes]

    sftA = region(L.sftA, 2 * m).view(np.int16).copy()
    sftB = region(L.sftB, 2 * n).view(np.int16).copy()
    A_lo = np.zeros((parts, nm, m, k), np.uint8)
    B_lo = np.zeros((parts, nm, n, k), np.uint8)
    for p in range(parts):
        for q in range(nm):
            if L.lo_format == 1:  # FP6 panel images: decode to the integers and re-encode as the e4m3 bytes the oracle holds (zero as +0)
                va = f6_plane_values(region(L.A_lo + p * L.part_strideA + q * L.sizeA, L.sizeA), m, L.mp, L.kp)
                vb = f6_plane_values(region(L.B_lo + p * L.part_strideB + q * L.sizeB, L.sizeB), n, n, L.kp)
                assert not va[:, k:].any() and not vb[:, k:].any(), "k-padding of the FP6 planes must be zero"
                A_lo[p, q] = e4m3_of_ints(va[:, :k])
                B_lo[p, q] = e4m3_of_ints(vb[:, :k])
                continue
            pa = region(L.A_lo + p * L.part_strideA + q * L.sizeA, L.sizeA).reshape(L.mp, L.kp)
            A_lo[p, q] = pa[:m, :k]
            assert not pa[:m, k:].any(), "k-padding of A_lo must be zero"
            pb = region(L.B_lo + p * L.part_strideB + q * L.sizeB, L.sizeB).reshape(n, L.kp)
            B_lo[p, q] = pb[:, :k]
            assert not pb[:, k:].any(), "k-padding of B_lo must be zero"
    mid_dt = np.int8 if backend == g.INT8 else np.int16
    comps = 2 if cplx else 1
    isz = np.dtype(mid_dt).itemsize * comps
    Cm = np.zeros((N, n, m, comps), mid_dt)
    for t in range(N):
        pc = region(L.C_mid + t * L.sizeC * isz, L.sizeC * isz).view(mid_dt).reshape(n, L.mp, comps)
        Cm[t] = pc[:, :m, :]
    if not cplx:
        Cm = Cm[..., 0]
    return dict(sftA=sftA, sftB=sftB, A_lo=A_lo, B_lo=B_lo, C_mid=Cm, lo_format=int(L.lo_format))


def hip_gemm(A, B, N, fastmode=False, backend=g.INT8, opA="N", opB="N", alpha=1.0, beta=0.0, C0=None, want_intermediates=False,
             timers=False):
    """A, B: numpy arrays as stored (before op), like oracle_lib.gemm.  Returns C (numpy m x n) [, intermediates]."""
    dA, dB = to_dev(A), to_dev(B)
    dC = to_dev(C0.copy()) if C0 is not None else None
    m, k = (A.shape if opA == "N" else A.shape[::-1])
    n = B.shape[1] if opB == "N" else B.shape[0]
    cplx = A.dtype.kind == "c"
    tot, _, _ = g.work_size(cplx, backend, m, n, k, N)
    work = torch.zeros(tot, dtype=torch.uint8, device="cuda")
    Cd, tm, work = g.gemm(dA, dB, N, fastmode=fastmode, backend=backend, opA=opA, opB=opB, alpha=alpha, beta=beta, C_out=dC,
                          work=work, timers=timers)
    torch.cuda.synchronize()
    Cn = from_dev(Cd)
    if not want_intermediates:
        return (Cn, tm) if timers else Cn
    inter = read_intermediates(work, g._dtype_code(dA.dtype), backend, m, n, k, N)
    return (Cn, inter, tm) if timers else (Cn, inter)


def bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def shifts_close(dev, orc, what=""):
    """Device vs oracle shifts: identical except for rare +-1 at floor boundaries of the log2 approximation."""
    d = dev.astype(int) - orc.astype(int)
    bad = np.abs(d) > 1
    assert not bad.any(), f"{what}: shift differs by more than 1 at {np.nonzero(bad)[0][:5]}"
    nd = int((d != 0).sum())
    assert nd <= max(1, 0.02 * d.size), f"{what}: {nd}/{d.size} shifts differ from the oracle (log2 boundary cases should be rare)"
    return nd


def bounds_case(A, B, N, opA="N", opB="N", backend=g.INT8, skip_layout=False, bound_mode=SAFE):
    """Accurate-mode scaling phase, first half, BIT-EXACT against the oracle (rows a3 / a4 of SURVEY.md section 8):
    the 7-bit (INT8) / e4m3 round-up (FP8) bound planes of both operands, the preliminary shifts sft0 = maxUFP - ilogb(amax)
    and the row / column maxima of the bound product (int32; FP8: inflated floats), read from the workspace right after
    gemmul8_scale_bounds (scaling_accu_real.hpp:23-136,415-432, scaling.hpp:3-94, find_max.hpp:67-114).
    skip_layout: carve the workspace with enable_skip_scalA/B = 1, where the bound planes have their own slot behind the
    residue planes (gemmul8_real.hpp:101-104) instead of aliasing plane 0.
    bound_mode (FP8 backend): SAFE = the product's engine-safe inflation, REFERENCE = (k+1)*2^-24 of find_max.hpp:82-96; selected on both sides."""
    if backend == g.FP8:
        select_fp8_bound_mode(bound_mode)
    dA, dB = to_dev(A), to_dev(B)
    m, k = (A.shape if opA == "N" else A.shape[::-1])
    n = B.shape[1] if opB == "N" else B.shape[0]
    cplx = A.dtype.kind == "c"
    en = int(skip_layout)
    tot, _, _ = g.work_size(cplx, backend, m, n, k, N, en, en)
    work = torch.full((tot,), 0x5A, dtype=torch.uint8, device="cuda")
    L = g.Layout()
    code = g._dtype_code(dA.dtype)
    lib = g.lib()
    g.check(lib.gemmul8_get_layout(code, backend, m, n, k, N, work.data_ptr(), None, None, en, en, C.byref(L)))
    st = torch.cuda.current_stream().cuda_stream
    g.check(lib.gemmul8_scale_bounds(st, code, backend, g.OPS[opA], g.OPS[opB], m, n, k, dA.data_ptr(), dA.shape[1], dB.data_ptr(),
                                     dB.shape[1], N, 0, n, C.byref(L), 0, 0), "scale_bounds")
    torch.cuda.synchronize()
    w = work.cpu().numpy()
    base = work.data_ptr()
    parts = 3 if cplx else 1

    def planes(ptr, rows, rows_alloc, plane_bytes):
        out = np.zeros((parts, rows, k), np.uint8)
        for p in range(parts):
            off = ptr - base + p * plane_bytes
            pl = w[off:off + rows_alloc * L.kp].reshape(rows_alloc, L.kp)
            out[p] = pl[:rows, :k]
            assert not pl[:rows, k:].any(), "k-padding of a bound plane must be zero"
        return out
    Ab = planes(L.A_bound, m, L.mp, L.sizeA)
    Bb = planes(L.B_bound, n, n, L.sizeB)
    s0A = w[L.sftA - base:L.sftA - base + 2 * m].view(np.int16)
    s0B = w[L.sftB - base:L.sftB - base + 2 * n].view(np.int16)
    np_ = (n + 255) // 256 * 256
    mx = w[L.scratch - base:L.scratch - base + 4 * (L.mp + np_)]
    mdt = np.int32 if backend == g.INT8 else np.float32
    rmax, cmax = mx[:4 * m].view(mdt), mx[4 * L.mp:4 * L.mp + 4 * n].view(mdt)
    oA, o0A = ol.extract_bounds(A, opA, True, backend)
    oB, o0B = ol.extract_bounds(B, opB, False, backend)
    assert np.array_equal(Ab, oA), f"A bound planes differ in {np.sum(Ab != oA)} bytes"
    assert np.array_equal(Bb, oB), f"B bound planes differ in {np.sum(Bb != oB)} bytes"
    assert np.array_equal(s0A, o0A) and np.array_equal(s0B, o0B), "preliminary shifts sft0 differ"
    orm, ocm = ol.bound_maxima(oA, oB, backend)
    if backend == g.INT8:
        assert np.array_equal(rmax, orm), f"row maxima of the bound GEMM differ at {np.nonzero(rmax != orm)[0][:5]}"
        assert np.array_equal(cmax, ocm), f"column maxima of the bound GEMM differ at {np.nonzero(cmax != ocm)[0][:5]}"
        return 0
    # FP8: the accumulation of the e4m3 products belongs to the ENGINE (the reference leaves it to the vendor's FP8 GEMM and
    # inflates by (k+1)*2^-24, find_max.hpp:82-96, an IEEE FP32 summation bound).  gfx950's v_mfma_scale_f32_16x16x128_f8f6f4 does
    # not add like that (tools/ubench/f8_accum.hip, profiles/archive/r02_f8_mfma_accumulation.txt): the 128 products of an instruction are
    # summed in groups of 8, inside a group everything is aligned to the largest product and bits below 2^-13 of it are dropped;
    # group sums and the accumulator are added with ~22 bits, truncating.  A non-negative sum therefore comes out equal to the
    # exact one or LOW (1.2e-3 seen in a 1500-seed fuzz sweep), or above it by a few ulp only (<= 15 ulp over 18 K-steps in the
    # round-4 24000-case stress sweep: the accumulator add is not a pure truncation, at most about one ulp up per K-step;
    # tools/f8_bound_stress_dbg.py prints such cases).  The product's default inflation
    # ku = 7*2^-13 + 4(k+1)*2^-24 (gemmul8_set_fp8_bound_mode) covers that loss; what is asserted for real types is the GUARANTEE:
    # exact un-inflated maximum <= device value <= the oracle's inflated value of the exactly accumulated sum (+ one ulp per K-step).
    if bound_mode == REFERENCE:
        # the reference's formula on this engine: nothing is guaranteed one-sidedly (that is why it is not the product's default) -- the device's
        # maxima sit within the engine's accumulation loss (1.2e-3 seen; 2^-9 allowed) of the oracle's inflated exactly-accumulated values
        for d, o, what in ((rmax, orm, "row"), (cmax, ocm, "column")):
            d64, o64 = d.astype(np.float64), o.astype(np.float64)
            assert np.all(np.abs(d64 - o64) <= 2.0 ** -9 * np.abs(o64)), f"{what} maxima of the FP8 bound GEMM (reference formula) off by {np.max(np.abs(d64 - o64) / np.maximum(np.abs(o64), 1e-300))}"
        return int((rmax != orm).sum() + (cmax != ocm).sum())
    if not cplx:
        ex_r, ex_c = ol.bound_maxima_f8_exact(oA, oB)
        for d, o, ex, what in ((rmax, orm, ex_r, "row"), (cmax, ocm, ex_c, "column")):
            d64 = d.astype(np.float64)
            assert np.all(d64 >= ex), f"{what} maxima of the FP8 bound GEMM BELOW the exact sum by {np.min((d64 - ex) / np.maximum(ex, 1e-300))}"
            assert np.all(d64 <= o.astype(np.float64) * (1 + (L.kp // 128 + 4) * 2.0 ** -23)), f"{what} maxima of the FP8 bound GEMM above the inflated exact sum"
        return int((rmax != orm).sum() + (cmax != ocm).sum())
    # complex (round 4): T = C0 + C1 with C0 = (|Ar|-|Ai|)(|Br|-|Bi|) of both signs.  The default combination inflates C0 by
    # ku (|C0| + 2 s12) (oz2_gemm_f8.hip bound_ku), which covers the engine's loss on the MAGNITUDES of C0's terms, so the same one-sided
    # GUARANTEE holds: exact un-inflated max(T, C1) <= device value.  Above, the device may exceed the oracle's inflated value of the exact
    # sums by what the engine loses on C0's NEGATIVE terms (at most eps (T + C1), inflated again): a 2^-9 band.
    ex_r, ex_c = ol.bound_maxima_f8_exact_cplx(oA, oB)
    for d, o, ex, what in ((rmax, orm, ex_r, "row"), (cmax, ocm, ex_c, "column")):
        d64 = d.astype(np.float64)
        assert np.all(d64 >= ex), f"{what} maxima of the complex FP8 bound BELOW the exact sum by {np.min((d64 - ex) / np.maximum(ex, 1e-300))}"
        assert np.all(d64 <= o.astype(np.float64) * (1 + 2.0 ** -9)), f"{what} maxima of the complex FP8 bound above the oracle's inflated value"
    return int((rmax != orm).sum() + (cmax != ocm).sum())


def parity_case(A, B, N, fastmode, opA="N", opB="N", alpha=1.0, beta=0.0, C0=None, backend=g.INT8, bound_mode=SAFE):
    """Full bit-exact parity of one case: accurate mode's bound planes / sft0 / bound maxima (exact), shifts (tolerant),
    planes, C_mid, C (exact given the device's shifts).  FP8 backend: `bound_mode` is selected on BOTH sides (SAFE = the product's
    default inflation, REFERENCE = the reference's formula = the oracle's default)."""
    if backend == g.FP8:
        select_fp8_bound_mode(bound_mode)
    if not fastmode:
        bounds_case(A, B, N, opA=opA, opB=opB, backend=backend, bound_mode=bound_mode)
    Cd, it = hip_gemm(A, B, N, fastmode=fastmode, backend=backend, opA=opA, opB=opB, alpha=alpha, beta=beta, C0=C0, want_intermediates=True)
    # oracle with its own shifts -> compare shifts
    _, ito = ol.gemm(A, B, N, fastmode=fastmode, backend=backend, opA=opA, opB=opB, alpha=alpha, beta=beta, C0=C0, want_intermediates=True)
    nd = shifts_close(it["sftA"], ito["sftA"], "sftA") + shifts_close(it["sftB"], ito["sftB"], "sftB")
    # oracle fed with the device's shifts -> everything downstream is bit-exact
    Co, ito = ol.gemm(A, B, N, fastmode=fastmode, backend=backend, opA=opA, opB=opB, alpha=alpha, beta=beta, C0=C0,
                      sftA_in=it["sftA"], sftB_in=it["sftB"], want_intermediates=True)
    if it["lo_format"] == 1:  # the FP6 images are compared as INTEGERS (f6_plane_values: a zero decodes to 0 whichever sign bit its code carries -- the four-k writer emits +0, the
        # hardware pack of the lane-per-fragment writer keeps the sign of a -0): the oracle's -0 byte (rint of a small negative quotient) compares as +0
        for key in ("A_lo", "B_lo"):
            ito[key] = np.where(ito[key] == 0x80, 0, ito[key]).astype(np.uint8)
    assert np.array_equal(it["A_lo"], ito["A_lo"]), "A_lo planes differ"
    assert np.array_equal(it["B_lo"], ito["B_lo"]), "B_lo planes differ"
    assert np.array_equal(it["C_mid"], ito["C_mid"]), "C_mid planes differ"
    assert bits_equal(Cd, Co), f"final C differs in {np.sum(Cd != Co)} elements"
    return nd


def embed(M, ld_extra, base_off, rng, tail=5):
    """Column-major matrix M (numpy rows x cols) placed inside a larger 1-D buffer of its element type: base offset `base_off` ELEMENTS
    (so the base pointer is only element-aligned), leading dimension rows + ld_extra, `tail` elements behind the last column; every element outside the window holds
    random finite garbage.  Returns (buffer, ld)."""
    rows, cols = M.shape
    ld = rows + ld_extra
    size = base_off + ld * cols + tail
    buf = (rng.random(size) * 1e3 - 500).astype(M.dtype)
    if M.dtype.kind == "c":
        buf = (buf + 1j * (rng.random(size) * 1e3 - 500)).astype(M.dtype)
    win = buf[base_off:base_off + ld * cols].reshape(cols, ld)
    win[:, :rows] = M.T
    return buf, ld


def window_mask(size, base_off, ld, rows, cols):
    """Boolean mask over a buffer of `embed`: True inside the rows x cols window."""
    mk = np.zeros(size, bool)
    mk[base_off:base_off + ld * cols].reshape(cols, ld)[:, :rows] = True
    return mk


def parity_case_embedded(A, B, C0, N, fastmode, opA, opB, alpha, beta, backend, ld_extra, base_off, rng, bound_mode=SAFE):
    """`parity_case` on sub-matrix views: A, B, C0 (numpy, as stored) are embedded in larger buffers with ld = rows + ld_extra and a base
    pointer `base_off` elements into the allocation; the HIP path (C ABI, explicit lda / ldb / ldc) and the oracle
    (oracle_lib.gemm_embedded) run on the same bytes.  Asserted: shifts (tolerant), then with the device's shifts planes / C_mid and
    the WHOLE C buffer bit for bit -- i.e. the m x n window equals the oracle's and every byte outside it is untouched; A's and B's
    buffers unchanged.  beta != 0 updates C in place inside the larger matrix."""
    if backend == g.FP8:
        select_fp8_bound_mode(bound_mode)
    m, k = (A.shape if opA == "N" else A.shape[::-1])
    n = B.shape[1] if opB == "N" else B.shape[0]
    exa, exb, exc = (ld_extra if np.ndim(ld_extra) else (ld_extra,) * 3)
    offa, offb, offc = (base_off if np.ndim(base_off) else (base_off,) * 3)
    bufA, lda = embed(A, exa, offa, rng)
    bufB, ldb = embed(B, exb, offb, rng)
    bufC, ldc = embed(C0, exc, offc, rng)
    dt = A.dtype
    cplx = dt.kind == "c"
    code = ol.DT[dt]
    dA, dB, dC = (torch.from_numpy(x.copy()).cuda() for x in (bufA, bufB, bufC))
    tot, _, _ = g.work_size(cplx, backend, m, n, k, N)
    work = torch.zeros(tot, dtype=torch.uint8, device="cuda")
    al, be = np.array([alpha], dtype=dt), np.array([beta], dtype=dt)
    isz = dt.itemsize
    rc = g.lib().gemmul8_gemm(torch.cuda.current_stream().cuda_stream, code, backend, g.OPS[opA], g.OPS[opB], m, n, k, al.ctypes.data,
                              dA.data_ptr() + offa * isz, lda, dB.data_ptr() + offb * isz, ldb, be.ctypes.data, dC.data_ptr() + offc * isz, ldc, N,
                              int(fastmode), work.data_ptr(), None, None, 0, 0, 0, 0, None)
    g.check(rc, "gemmul8_gemm")
    torch.cuda.synchronize()
    it = read_intermediates(work, code, backend, m, n, k, N)
    assert bits_equal(dA.cpu().numpy(), bufA) and bits_equal(dB.cpu().numpy(), bufB), "an operand buffer was written"
    Cdev = dC.cpu().numpy()
    # the oracle with its own shifts (shift comparison), then with the device's (everything downstream bit-exact)
    oC = bufC.copy()
    ito = ol.gemm_embedded(bufA, offa, lda, bufB, offb, ldb, oC, offc, ldc, m, n, k, N, fastmode, backend, opA, opB, alpha, beta)
    nd = shifts_close(it["sftA"], ito["sftA"], "sftA") + shifts_close(it["sftB"], ito["sftB"], "sftB")
    oC = bufC.copy()
    ito = ol.gemm_embedded(bufA, offa, lda, bufB, offb, ldb, oC, offc, ldc, m, n, k, N, fastmode, backend, opA, opB, alpha, beta,
                           sftA_in=it["sftA"], sftB_in=it["sftB"])
    if it["lo_format"] == 1:
        for key in ("A_lo", "B_lo"):
            ito[key] = np.where(ito[key] == 0x80, 0, ito[key]).astype(np.uint8)
    assert np.array_equal(it["A_lo"], ito["A_lo"]), "A_lo planes differ"
    assert np.array_equal(it["B_lo"], ito["B_lo"]), "B_lo planes differ"
    assert np.array_equal(it["C_mid"], ito["C_mid"]), "C_mid planes differ"
    mk = window_mask(bufC.size, offc, ldc, m, n)
    assert bits_equal(Cdev[~mk], bufC[~mk]), "bytes of the enclosing C buffer outside the m x n window were written"
    assert bits_equal(oC[~mk], bufC[~mk])
    assert bits_equal(Cdev[mk], oC[mk]), f"final C differs in {np.sum(Cdev[mk] != oC[mk])} elements"
    return nd, it["lo_format"]


# ---- the rank-k entry points (gemmul8_syrk / gemmul8_herk / gemmul8_syr2k): one driver, and the three checks of their suites
RANK_K = ("syrk", "herk", "syr2k")
SENTINEL = 0xA5
LDC_EXTRA = (1, 7, 64)


def pad256(k):
    return (k + 255) // 256 * 256


def rank_k_inner(routine, k):
    """inner dimension of the GEMM whose workspace layout (and oracle cost) a rank-k call has"""
    return 2 * pad256(k) if routine == "syr2k" else k


def rank_k_work_size(routine, cplx, n, k, N):
    return g.work_size(cplx, g.INT8, n, n, rank_k_inner(routine, k), N)[0]


def tri_mask(n, uplo):
    """[row][col]: True inside the stored triangle, diagonal included"""
    i, j = np.indices((n, n))
    return i >= j if uplo == "L" else i <= j


def rank_k_call(routine, dt, n, k, uplo, trans, N, fast, alpha, beta, dA, lda, dC, ldc, dB=None, ldb=0, offA=0, offB=0, offC=0, scalars_dev=False, work=None):
    """One call of a rank-k C entry point.  dA, dB, dC: device tensors that hold the buffers the operands live in (any shape and element type; `dC` comes in
    sentinel-filled, see sentinel_c, and is updated in place); lda / ldb / ldc and the base offsets off* are in ELEMENTS of `dt`.  alpha, beta: python
    scalars, passed as host or device pointers of the routine's scalar type (HERK: the real type of `dt`'s width).  Returns the workspace (a fresh one,
    filled with 0x3C, unless given); the caller synchronises."""
    dt = np.dtype(dt)
    esz = dt.itemsize
    sdt = np.dtype(np.float32 if esz == 8 else np.float64) if routine == "herk" else dt
    al, be = np.array([alpha], dtype=sdt), np.array([beta], dtype=sdt)
    keep = (al, be)
    if scalars_dev:
        keep = (torch.from_numpy(al).cuda(), torch.from_numpy(be).cuda())
        pa, pb = keep[0].data_ptr(), keep[1].data_ptr()
    else:
        pa, pb = al.ctypes.data, be.ctypes.data
    if work is None:
        work = torch.full((rank_k_work_size(routine, dt.kind == "c", n, k, N),), 0x3C, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    head = (st, ol.DT[dt], g.INT8, g.UPLO[uplo], g.OPS[trans], n, k, pa, dA.data_ptr() + offA * esz, lda)
    tail = (pb, dC.data_ptr() + offC * esz, ldc, N, int(fast), work.data_ptr(), None)
    if routine == "syr2k":
        rc = g.lib().gemmul8_syr2k(*head, dB.data_ptr() + offB * esz, ldb, *tail)
    else:
        rc = getattr(g.lib(), "gemmul8_" + routine)(*head, *tail)
    g.check(rc, "gemmul8_" + routine)
    if scalars_dev:
        torch.cuda.synchronize()   # the device scalars stay alive until the call has read them
    return work


def sentinel_c(C0, uplo, ld_extra, off=0, tail=3):
    """The C buffer of a rank-k call: off + (n + ld_extra) * n + tail elements, every byte SENTINEL except the triangle `uplo` of the n x n window at element
    `off`, which holds C0's.  Returns (bytes uint8 [elements][esz], ldc, inside) with inside[element] True on the triangle's elements."""
    n = C0.shape[0]
    esz = C0.dtype.itemsize
    ldc = n + ld_extra
    buf = np.full((off + ldc * n + tail, esz), SENTINEL, np.uint8)
    inside = np.zeros(buf.shape[0], bool)
    mk = tri_mask(n, uplo)
    inside[off:off + ldc * n].reshape(n, ldc)[:, :n] = mk.T
    buf[off:off + ldc * n].reshape(n, ldc, esz)[:, :n][mk.T] = np.ascontiguousarray(C0.T).view(np.uint8).reshape(n, n, esz)[mk.T]
    return buf, ldc, inside


def rank_k_equivalent(routine, A, B, trans):
    """(P, Q, opP, opQ): the GEMM a rank-k call is defined by -- SYRK A A^T, HERK A A^H, SYR2K the K-concatenated P Q^T of tests/test_syr2k_premise.py"""
    if routine == "syr2k":
        from test_syr2k_premise import concat
        P, Q, _ = concat(A, B, trans)
        return P, Q, trans, "T" if trans == "N" else "N"
    return A, A, trans, ("C" if routine == "herk" else "T") if trans == "N" else "N"


def window_bytes(out, n, ldc, off):
    """the n x n window of a C buffer's bytes as [col][row][esz]"""
    return out[off:off + ldc * n].reshape(n, ldc, -1)[:, :n]


def triangle_differs(routine, got, ref, uplo):
    """(a) / (b): [col][row] mask of the stored triangle's entries whose bytes differ from the GEMM's `ref` (numpy n x n).  HERK: the diagonal is compared
    in its real part only, and its imaginary part must be all-zero bits (+0.0)."""
    n = ref.shape[0]
    esz = ref.dtype.itemsize
    refb = np.ascontiguousarray(ref.T).view(np.uint8).reshape(n, n, esz)
    ne = got != refb
    if routine == "herk":
        d = np.arange(n)
        assert not got[d, d, esz // 2:].any(), "a diagonal imaginary part is not +0.0"
        ne[d, d, esz // 2:] = False
    return ne.any(axis=2) & tri_mask(n, uplo).T


def _rank_k_marked_work(routine, code, n, k, N):
    """A workspace whose every byte is 0x3C -- so that zero padding and SYR2K's zero block read as zero only if the call wrote them -- but for the plane sets
    of the equivalent GEMM's B_lo that the routine never writes (SYRK: all, HERK: part 0), which read_intermediates expects zero"""
    cplx = code >= 2
    kk = rank_k_inner(routine, k)
    work = torch.full((g.work_size(cplx, g.INT8, n, n, kk, N)[0],), 0x3C, dtype=torch.uint8, device="cuda")
    L = g.Layout()
    g.check(g.lib().gemmul8_get_layout(code, g.INT8, n, n, kk, N, work.data_ptr(), None, None, 0, 0, C.byref(L)))
    for p in range({"syrk": L.parts, "herk": 1, "syr2k": 0}[routine]):
        off = L.B_lo + p * L.part_strideB - work.data_ptr()
        work[off:off + L.num_mat * L.sizeB] = 0
    return work


def rank_k_case(routine, A, B, C0, uplos, trans, N, fast, alpha, beta, ld_extra=(0, 0, 1), base_off=(0, 0, 0), scalars_dev=False, oracle=True, rng=None,
                nan_diag=True, intermediates=False, gemm=True):
    """The three checks of the rank-k suites on one case, every `uplo` of `uplos` against ONE equivalent GEMM: (a) the stored triangle equals gemmul8_gemm
    run in the same process, (b) (oracle=True) it equals the CPU oracle's GEMM fed with the device GEMM's shifts, and that GEMM's C is finite, (c) every
    byte of the sentinel-filled C buffer outside the triangle is unchanged; and the buffers A and B are embedded in (ld = rows + ld_extra, base offset in
    elements, random finite data around them) are byte-identical after the call.  A, B (None but for SYR2K; `B is A` passes the same pointer), C0: numpy,
    as stored.  HERK: C0's diagonal is real and, with nan_diag, the call sees NaN in the diagonal's imaginary parts.  gemm=False: no GEMM, (c) and the
    operand buffers only (a caller that compares two runs of the same call).  Returns {"out": {uplo: bytes of the C buffer after the call}, "tri": {uplo:
    [col][row] mask}, "it": {uplo: the call's intermediates in its own layout, with intermediates=True -- which also
    holds its shifts and planes against the equivalent GEMM's}, "gemm": the device GEMM's C}."""
    rng = rng or np.random.default_rng(1)
    dt = A.dtype
    n, k = A.shape if trans == "N" else A.shape[::-1]
    exa, exb, exc = ld_extra
    offa, offb, offc = base_off
    bufA, lda = embed(A, exa, offa, rng)
    dA = torch.from_numpy(bufA.copy()).cuda()
    if routine == "syr2k" and B is not A:
        bufB, ldb = embed(B, exb, offb, rng)
        dB = torch.from_numpy(bufB.copy()).cuda()
    else:
        bufB, ldb, dB, offb = bufA, lda, dA, offa
    assert not oracle or gemm
    Cg = Co = None
    if gemm:
        P, Q, opP, opQ = rank_k_equivalent(routine, A, B, trans)
        Cg = hip_gemm(P, Q, N, fastmode=fast, opA=opP, opB=opQ, alpha=alpha, beta=beta, C0=C0, want_intermediates=oracle or intermediates)
        if oracle or intermediates:
            Cg, itg = Cg
    if oracle:
        Co = np.asarray(ol.gemm(P, Q, N, fastmode=fast, opA=opP, opB=opQ, alpha=alpha, beta=beta, C0=C0, sftA_in=itg["sftA"], sftB_in=itg["sftB"]))
        assert np.isfinite(Co).all(), "the oracle's C is not finite: the case's data leaves the type's range"
    Cin = C0
    if routine == "herk" and nan_diag:
        Cin = C0.copy()
        Cin.imag[np.arange(n), np.arange(n)] = np.nan
    res = dict(out={}, tri={}, it={}, gemm=Cg)
    code = ol.DT[dt]
    for uplo in uplos:
        before, ldc, inside = sentinel_c(Cin, uplo, exc, offc)
        dC = torch.from_numpy(before.copy()).cuda()
        work = _rank_k_marked_work(routine, code, n, k, N) if intermediates else None
        work = rank_k_call(routine, dt, n, k, uplo, trans, N, fast, alpha, beta, dA, lda, dC, ldc, dB, ldb, offa, offb, offc, scalars_dev, work)
        torch.cuda.synchronize()
        out = dC.cpu().numpy()
        what = f"{routine} {dt.name} n={n} k={k} uplo={uplo} trans={trans} N={N} fast={fast} scalars=({alpha}, {beta}) ld={ld_extra} off={base_off}"
        assert bits_equal(dA.cpu().numpy(), bufA) and bits_equal(dB.cpu().numpy(), bufB), "an operand buffer was written: " + what
        assert np.array_equal(out[~inside], before[~inside]), "bytes outside the stored triangle were written: " + what                          # (c)
        got = window_bytes(out, n, ldc, offc)
        for ref, name in ((Cg, "the equivalent gemmul8_gemm"), (Co, "the oracle's GEMM")):                                                       # (a), (b)
            if ref is not None:
                bad = triangle_differs(routine, got, ref, uplo)
                assert not bad.any(), f"{bad.sum()} entries of the triangle differ from {name}, first at (col, row) {np.argwhere(bad)[:3].tolist()}: " + what
        res["out"][uplo] = got.copy()
        res["tri"][uplo] = tri_mask(n, uplo).T
        if intermediates:
            it = res["it"][uplo] = read_intermediates(work, code, g.INT8, n, n, rank_k_inner(routine, k), N)
            if gemm:   # the one operand pass leaves the equivalent GEMM's shifts and planes: all of A_lo; of B_lo what the routine does not alias (SYRK: nothing, HERK: parts 1, 2)
                assert np.array_equal(it["sftA"], itg["sftA"]) and np.array_equal(itg["sftB"], itg["sftA"]), "sftA differs from the equivalent GEMM's: " + what
                assert np.array_equal(it["A_lo"], itg["A_lo"]), "A_lo differs from the equivalent GEMM's: " + what
                first = {"syrk": 3, "herk": 1, "syr2k": 0}[routine]
                assert np.array_equal(it["B_lo"][first:], itg["B_lo"][first:]), "the right-hand planes differ from the equivalent GEMM's B_lo: " + what
                if routine == "herk":
                    assert not it["B_lo"][0].any(), "part 0 of B_lo, which HERK aliases to A_lo's, was written: " + what
    return res


# ---- gemmul8_gemm_batched on views (tests/test_gpu_batched_paths.py): one driver and its three checks
C_SENTINEL = {4: 0x7FC0BEEF, 8: 0x7FF8DEADBEEF0123}   # one fixed (quiet) NaN bit pattern per real component of the C buffer outside the windows
ITEM_SCALE_STEP, ITEM_SCALE_MOD = 3, 11               # item b's operands are scaled by 2^(3 b mod 11): no two of eleven consecutive items share shifts


def rand_spread(shape, dtype, rng):
    """entries of mixed magnitude (a log-normal spread), both signs; complex types in both components"""
    x = (rng.random(shape) - 0.5) * np.exp(rng.standard_normal(shape))
    if np.dtype(dtype).kind == "c":
        x = x + 1j * (rng.random(shape) - 0.5) * np.exp(rng.standard_normal(shape))
    return x.astype(dtype)


def stored_shape(op, rows, k):
    """shape of the matrix as stored whose op() is rows x k (B: op(B)^T is n x k, so stored_shape of the opposite op)"""
    return (rows, k) if op == "N" else (k, rows)


def batched_data(dt, m, n, k, batch, opA="N", opB="N", shareA=False, shareB=False, rng=None, gen=rand_spread):
    """Independent items as stored (numpy, before op): lists As, Bs (ONE entry for a shared operand, stride 0) and C0s.  Item b's own operands are scaled
    by s = 2^(3 b mod 11), its C0 by s^2: the items' shifts differ, so that a mixed-up item offset cannot cancel."""
    rng = rng or np.random.default_rng(0)
    dt = np.dtype(dt)
    sc = [2.0 ** (ITEM_SCALE_STEP * b % ITEM_SCALE_MOD) for b in range(batch)]
    shA, shB = stored_shape(opA, m, k), stored_shape("T" if opB == "N" else "N", n, k)
    As = [gen(shA, dt, rng)] if shareA else [(gen(shA, dt, rng) * s).astype(dt) for s in sc]
    Bs = [gen(shB, dt, rng)] if shareB else [(gen(shB, dt, rng) * s).astype(dt) for s in sc]
    C0s = [(gen((m, n), dt, rng) * s * s).astype(dt) for s in sc]
    return As, Bs, C0s


def _strided_buffer(items, count, pad, gap, head, fill, tail=4):
    """`count` column-major windows in one 1-D buffer of the items' type: ld = rows + pad, item b at element head + b * stride, stride = ld * cols + gap
    (0 when `items` holds the ONE matrix every item shares); every other element is `fill(size) -> array`.  Returns (buffer, ld, stride, inside mask)."""
    rows, cols = items[0].shape
    ld = rows + pad
    shared = len(items) == 1 and count > 1
    stride = 0 if shared else ld * cols + gap
    size = head + (len(items) - 1) * stride + ld * cols + tail
    buf = fill(size)
    inside = np.zeros(size, bool)
    for b, M in enumerate(items):
        o = head + b * stride
        buf[o:o + ld * cols].reshape(cols, ld)[:, :rows] = M.T
        inside[o:o + ld * cols].reshape(cols, ld)[:, :rows] = True
    return buf, ld, stride, inside


def _fill_operand(dt, nan):
    """what surrounds the windows of A and B: huge finite numbers of both signs, which would wreck the bounds and the residues if a kernel used one (non-finite
    mode 1: NaN, which would flag a row or a column)"""
    dt = np.dtype(dt)
    big = np.nan if nan else (1e30 if dt.itemsize // (2 if dt.kind == "c" else 1) == 4 else 1e300)

    def fill(size):
        v = np.full(size, big, dt)
        v[1::2] *= -1
        if dt.kind == "c":
            v = (v + 1j * v).astype(dt)
        return v
    return fill


def _fill_c(dt):
    dt = np.dtype(dt)
    rsz = dt.itemsize // (2 if dt.kind == "c" else 1)

    def fill(size):
        v = np.empty(size, dt)
        v.view(np.uint32 if rsz == 4 else np.uint64)[:] = C_SENTINEL[rsz]
        return v
    return fill


def work_vectors(work, code, backend, m, n, k, N, off=0, maxima=False):
    """The shifts one item's call left in its workspace block (`off` bytes behind the 256-aligned start of `work`), read through gemmul8_get_layout; with
    maxima (real INT8, accurate mode: the only case in which nothing reuses that scratch afterwards) also the bound GEMM's integer row and column maxima."""
    base = (work.data_ptr() + 255) // 256 * 256 + off
    L = g.Layout()
    g.check(g.lib().gemmul8_get_layout(code, backend, m, n, k, N, base, None, None, 0, 0, C.byref(L)))

    def vec(ptr, count, dt):
        o = ptr - work.data_ptr()
        return work[o:o + count * np.dtype(dt).itemsize].cpu().numpy().view(dt).copy()
    out = dict(sftA=vec(L.sftA, m, np.int16), sftB=vec(L.sftB, n, np.int16))
    if maxima:
        out["rowmax"], out["colmax"] = vec(L.scratch, m, np.int32), vec(L.scratch + 4 * L.mp, n, np.int32)
    return out


def _same_bits_nan(a, b):
    """bit-equal, any NaN matching any NaN (non-finite mode 1)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind == "c":
        rdt = np.float32 if a.dtype.itemsize == 8 else np.float64
        a, b = a.view(rdt), b.view(rdt)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint8), b[~nb].view(np.uint8))


def batched_views_case(As, Bs, C0s, N, fast, backend=g.INT8, opA="N", opB="N", alpha=1.0, beta=0.0, pad=(0, 0, 0), gap=(0, 0, 0), head=0, mode=0,
                       oracle_items=None, oracle_shifts=True, maxima=False, what=""):
    """ONE gemmul8_gemm_batched call on views, and the three checks of tests/test_gpu_batched_paths.py.

    As, Bs, C0s: the items as stored (numpy; `batched_data`), one entry in As / Bs for an operand every item shares (stride 0).  A, B and C live in larger
    device buffers: ld = rows + pad[i], stride = ld * cols + gap[i] (i = 0, 1, 2 for A, B, C), the first window `head` elements into the buffer.  Outside the
    windows the C buffer holds C_SENTINEL, the A and B buffers huge finite numbers (mode 1: NaN).  Asserted:
      (a) every item is bit-identical to a gemmul8_gemm call on the same views (mode 1: any NaN matches any NaN), and so are its shifts in the workspace
          (with maxima=True also the bound GEMM's integer maxima);
      (b) the items of `oracle_items` (default: first, middle, last; mode 1: none) are bit-identical to oracle_lib.gemm with the same ops, scalars, C0, mode and
          backend, fed with the shifts the BATCHED call left in that item's workspace block; for the first of them the oracle's own shifts are held against
          those (shifts_close: equal but for rare +-1 at the floor boundaries of the device's log2; oracle_shifts=False leaves that run out).  An item whose C0 holds a
          NaN or an Inf is compared with any NaN matching any NaN;
      (c) every byte of the C buffer outside the windows, and the whole A and B buffers, are unchanged.
    Returns {"C": the C buffer after the batched call (numpy), "windows": [m x n numpy per item], "vectors": [work_vectors per item]}."""
    batch = len(C0s)
    dt = C0s[0].dtype
    m, n = C0s[0].shape
    k = As[0].shape[1] if opA == "N" else As[0].shape[0]
    assert (Bs[0].shape == (k, n) if opB == "N" else Bs[0].shape == (n, k)) and len(As) in (1, batch) and len(Bs) in (1, batch)
    if backend == g.FP8:
        select_fp8_bound_mode(SAFE)
    cplx = dt.kind == "c"
    code, esz = ol.DT[dt], dt.itemsize
    bufA, lda, sA, _ = _strided_buffer(As, batch, pad[0], gap[0], head, _fill_operand(dt, mode == 1))
    bufB, ldb, sB, _ = _strided_buffer(Bs, batch, pad[1], gap[1], head, _fill_operand(dt, mode == 1))
    bufC, ldc, sC, inside = _strided_buffer([np.asarray(c) for c in C0s], batch, pad[2], gap[2], head, _fill_c(dt))
    dA, dB, dC, dC1 = (torch.from_numpy(x.copy()).cuda() for x in (bufA, bufB, bufC, bufC))
    pA, pB, pC, pC1 = (t.data_ptr() + head * esz for t in (dA, dB, dC, dC1))
    lib = g.lib()
    W = lib.gemmul8_batched_item_bytes(int(cplx), backend, m, n, k, N)
    work = torch.empty(lib.gemmul8_work_size_batched(int(cplx), backend, m, n, k, N, batch), dtype=torch.uint8, device="cuda")
    work1 = torch.empty(g.work_size(cplx, backend, m, n, k, N)[0], dtype=torch.uint8, device="cuda")
    al, be = np.array([alpha], dt), np.array([beta], dt)
    st = torch.cuda.current_stream().cuda_stream
    what = f"{what} {dt.name} backend={backend} {m}x{n}x{k} batch={batch} N={N} fast={fast} op={opA}{opB} scalars=({alpha}, {beta}) pad={pad} gap={gap} head={head} " \
           f"strides=({sA}, {sB}, {sC}) mode={mode}"
    prev = g.set_nonfinite_mode(mode)
    try:
        g.check(lib.gemmul8_gemm_batched(st, code, backend, g.OPS[opA], g.OPS[opB], m, n, k, al.ctypes.data, pA, lda, sA, pB, ldb, sB, be.ctypes.data, pC, ldc, sC,
                                         batch, N, int(fast), work.data_ptr()), "gemmul8_gemm_batched: " + what)
        torch.cuda.synchronize()
        vb = [work_vectors(work, code, backend, m, n, k, N, b * W, maxima) for b in range(batch)]
        v1 = []
        for b in range(batch):
            g.check(lib.gemmul8_gemm(st, code, backend, g.OPS[opA], g.OPS[opB], m, n, k, al.ctypes.data, pA + b * sA * esz, lda, pB + b * sB * esz, ldb,
                                     be.ctypes.data, pC1 + b * sC * esz, ldc, N, int(fast), work1.data_ptr(), None, None, 0, 0, 0, 0, None), "gemmul8_gemm: " + what)
            torch.cuda.synchronize()
            v1.append(work_vectors(work1, code, backend, m, n, k, N, 0, maxima))
    finally:
        g.set_nonfinite_mode(prev)
    got, per_item = dC.cpu().numpy(), dC1.cpu().numpy()
    assert bits_equal(dA.cpu().numpy(), bufA) and bits_equal(dB.cpu().numpy(), bufB), "an operand buffer was written: " + what                         # (c)
    assert bits_equal(got[~inside], bufC[~inside]), f"{int((got[~inside].view(np.uint8) != bufC[~inside].view(np.uint8)).sum())} bytes of the C buffer outside the windows were written: " + what
    assert bits_equal(per_item[~inside], bufC[~inside]), "a per-item call wrote outside its window: " + what

    def window(buf, b):
        return buf[head + b * sC:head + b * sC + ldc * n].reshape(n, ldc)[:, :m].T
    for b in range(batch):                                                                                                                              # (a)
        wb, w1 = window(got, b), window(per_item, b)
        same = _same_bits_nan(wb, w1) if mode == 1 else bits_equal(wb, w1)
        assert same, f"item {b}: {int((wb != w1).sum())} entries differ from the per-item call (NaN counted): " + what
        for key in vb[b]:
            assert np.array_equal(vb[b][key], v1[b][key]), f"item {b}: {key} in the workspace differs from the per-item call's at {np.nonzero(vb[b][key] != v1[b][key])[0][:5]}: " + what
    if oracle_items is None:
        oracle_items = sorted({0, batch // 2, batch - 1}) if mode == 0 else ()
    for i, b in enumerate(oracle_items):                                                                                                                # (b)
        A, B = As[b if len(As) > 1 else 0], Bs[b if len(Bs) > 1 else 0]
        kw = dict(fastmode=fast, backend=backend, opA=opA, opB=opB, alpha=alpha, beta=beta, C0=C0s[b])
        if i == 0 and oracle_shifts:
            _, ito = ol.gemm(A, B, N, want_intermediates=True, **kw)
            shifts_close(vb[b]["sftA"], ito["sftA"], f"item {b} sftA"), shifts_close(vb[b]["sftB"], ito["sftB"], f"item {b} sftB")
        Co = np.asarray(ol.gemm(A, B, N, sftA_in=vb[b]["sftA"], sftB_in=vb[b]["sftB"], **kw))
        finite_c0 = bool(np.isfinite(C0s[b]).all())
        assert np.isfinite(Co).all() or not finite_c0, "the oracle's C is not finite: the case's data leaves the type's range: " + what
        wb = window(got, b)
        assert bits_equal(wb, Co) if finite_c0 else _same_bits_nan(wb, Co), f"item {b}: {int((wb != Co).sum())} entries differ from the oracle, first at (row, col) {np.argwhere(wb != Co)[:3].tolist()}: " + what
    return dict(C=got, windows=[window(got, b).copy() for b in range(batch)], vectors=vb)
