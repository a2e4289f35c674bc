"""-m gpu: gemmul8_gemm_batched_ptr (a batch whose items are named by three DEVICE arrays of addresses, as ONE set of launches; the arrays are read
by the kernels only) against per-item gemmul8_gemm calls on the same addresses -- byte for byte, over the whole buffers the items live in, so that a
write outside a C window shows as well -- and one item per type against the oracle fed with the shifts the batched call left in that item's workspace.

What a host-side decision from an operand address would get wrong is what the cases are built around: items in shuffled address order, items of one
batch with different alignments, a C that is only element-aligned at the shape where the strided form takes the LDS-DMA CRT, the tall operands at which
a single call may take the one-read bound extract, shared operands, non-finite data in some items only, arrays written in stream order right before the
call, and a captured call replayed after the arrays' contents changed."""
import numpy as np
import pytest
import torch

import gemmul8_amd as g
import gpu_util as gu
import oracle_lib as ol

pytestmark = pytest.mark.gpu

CPLX_SCALARS = (-1.5 + 0.5j, 0.5 - 0.25j)   # on a real type the real parts


def scalars(dt):
    return CPLX_SCALARS if np.dtype(dt).kind == "c" else (CPLX_SCALARS[0].real, CPLX_SCALARS[1].real)


class Placed:
    """One operand of a batch: every item is a rows x cols column-major window with leading dimension `ld` somewhere in one of the `host` arrays (1-D, of the
    element type; `tens` are their device copies); where[b] = (array, element offset) of item b.  Items may name the same window."""

    def __init__(self, host, where, rows, cols, ld):
        self.host, self.where, self.rows, self.cols, self.ld = host, where, rows, cols, ld
        self.tens = [torch.from_numpy(h.copy()).cuda() for h in host]

    def addrs(self):
        esz = self.host[0].dtype.itemsize
        return [self.tens[a].data_ptr() + off * esz for a, off in self.where]

    def twin(self):
        """the same placement in fresh device buffers with the initial contents"""
        return Placed(self.host, self.where, self.rows, self.cols, self.ld)

    def window(self, arrays, b):
        a, off = self.where[b]
        return arrays[a][off:off + self.ld * self.cols].reshape(self.cols, self.ld)[:, :self.rows].T

    def outside(self):
        masks = [np.ones(h.size, bool) for h in self.host]
        for b in range(len(self.where)):
            self.window(masks, b)[...] = False
        return masks

    def download(self):
        return [t.cpu().numpy() for t in self.tens]


def filler(dt, size, c):
    """what lies around the windows: huge finite numbers around A and B, a byte pattern around C"""
    dt = np.dtype(dt)
    if c:
        return np.frombuffer(bytes([0xA5]) * (size * dt.itemsize), dtype=dt).copy()
    big = np.full(size, 3.0e30 if dt.itemsize // (2 if dt.kind == "c" else 1) == 4 else 7.0e300)
    return (big * (1 + 1j) if dt.kind == "c" else big).astype(dt)


def place(mats, pad=0, shift=None, separate=False, c=False, order=None, tail=5):
    """mats: the items as rows x cols numpy matrices (an item that IS another item's matrix shares its window).  ld = rows + pad.
    separate: every item in an allocation of its own, allocated in the order `order` (so that addresses do not ascend with the item index); otherwise all
    items in one buffer, item b's first element `shift[b]` elements behind a 16-byte boundary."""
    rows, cols = mats[0].shape
    dt = mats[0].dtype
    ld = rows + pad
    span = ld * cols
    batch = len(mats)
    shift = shift or [0] * batch
    per16 = max(1, 16 // dt.itemsize)
    first = {}
    host, where = [], [None] * batch
    if separate:
        for b in (order or range(batch)):
            if id(mats[b]) in first:
                where[b] = first[id(mats[b])]
                continue
            h = filler(dt, shift[b] + span + tail, c)
            host.append(h)
            where[b] = first[id(mats[b])] = (len(host) - 1, shift[b])
    else:
        cursor = 0
        for b in range(batch):
            if id(mats[b]) in first:
                where[b] = first[id(mats[b])]
                continue
            cursor = (cursor + per16 - 1) // per16 * per16 + per16 + shift[b]
            where[b] = first[id(mats[b])] = (0, cursor)
            cursor += span + 3
        host = [filler(dt, cursor + tail, c)]
    P = Placed.__new__(Placed)
    P.host, P.where, P.rows, P.cols, P.ld = host, where, rows, cols, ld
    for b in range(batch):
        P.window(host, b)[...] = mats[b]
    return Placed(host, where, rows, cols, ld)


def dev_array(addrs):
    return torch.tensor(addrs, dtype=torch.int64).cuda()


def call_ptr(dt, backend, opA, opB, m, n, k, alpha, beta, arrA, lda, arrB, ldb, arrC, ldc, batch, N, fast, work, stream=None):
    dt = np.dtype(dt)
    al, be = np.array([alpha], dt), np.array([beta], dt)
    st = stream if stream is not None else torch.cuda.current_stream().cuda_stream
    g.check(g.lib().gemmul8_gemm_batched_ptr(st, ol.DT[dt], backend, g.OPS[opA], g.OPS[opB], m, n, k, al.ctypes.data, arrA.data_ptr(), lda, arrB.data_ptr(), ldb,
                                             be.ctypes.data, arrC.data_ptr(), ldc, batch, N, int(fast), work.data_ptr()), "gemmul8_gemm_batched_ptr")


def call_items(dt, backend, opA, opB, m, n, k, alpha, beta, pA, lda, pB, ldb, pC, ldc, N, fast):
    dt = np.dtype(dt)
    al, be = np.array([alpha], dt), np.array([beta], dt)
    st = torch.cuda.current_stream().cuda_stream
    work1 = torch.empty(g.work_size(dt.kind == "c", backend, m, n, k, N)[0], dtype=torch.uint8, device="cuda")
    for a, b, c in zip(pA, pB, pC):
        g.check(g.lib().gemmul8_gemm(st, ol.DT[dt], backend, g.OPS[opA], g.OPS[opB], m, n, k, al.ctypes.data, a, lda, b, ldb, be.ctypes.data, c, ldc, N, int(fast),
                                     work1.data_ptr(), None, None, 0, 0, 0, 0, None), "gemmul8_gemm")
    torch.cuda.synchronize()


def batch_work(dt, backend, m, n, k, N, batch):
    return torch.empty(g.lib().gemmul8_work_size_batched(int(np.dtype(dt).kind == "c"), backend, m, n, k, N, batch), dtype=torch.uint8, device="cuda")


def ptr_case(As, Bs, C0s, N, fast, backend=g.INT8, opA="N", opB="N", alpha=None, beta=None, PA=None, PB=None, PC=None, mode=0, oracle_item=None, what=""):
    """ONE gemmul8_gemm_batched_ptr call against per-item gemmul8_gemm calls on twins of the C buffers.  Asserted: the C buffers are equal byte for byte
    (mode 1: any NaN matches any NaN), nothing outside the C windows changed, A and B are unchanged; oracle_item: that item equals oracle_lib.gemm fed with
    the shifts the batched call left in its workspace block, bit for bit."""
    dt = C0s[0].dtype
    m, n = C0s[0].shape
    batch = len(C0s)
    k = As[0].shape[1] if opA == "N" else As[0].shape[0]
    if alpha is None:
        alpha, beta = scalars(dt)
    PA, PB, PC = PA or place(As, separate=True), PB or place(Bs, separate=True), PC or place(C0s, separate=True, c=True)
    PC1 = PC.twin()
    work = batch_work(dt, backend, m, n, k, N, batch)
    arrA, arrB, arrC = dev_array(PA.addrs()), dev_array(PB.addrs()), dev_array(PC.addrs())
    what = f"{what} {dt.name} backend={backend} {m}x{n}x{k} batch={batch} N={N} fast={fast} op={opA}{opB} ld=({PA.ld}, {PB.ld}, {PC.ld}) mode={mode}"
    prev = g.set_nonfinite_mode(mode)
    try:
        call_ptr(dt, backend, opA, opB, m, n, k, alpha, beta, arrA, PA.ld, arrB, PB.ld, arrC, PC.ld, batch, N, fast, work)
        torch.cuda.synchronize()
        call_items(dt, backend, opA, opB, m, n, k, alpha, beta, PA.addrs(), PA.ld, PB.addrs(), PB.ld, PC1.addrs(), PC1.ld, N, fast)
    finally:
        g.set_nonfinite_mode(prev)
    got, ref = PC.download(), PC1.download()
    same = gu._same_bits_nan if mode == 1 else gu.bits_equal
    for i, (x, y, h, out) in enumerate(zip(got, ref, PC.host, PC.outside())):
        assert gu.bits_equal(x[out], h[out]), f"C buffer {i}: {int((x[out].view(np.uint8) != h[out].view(np.uint8)).sum())} bytes outside the windows were written: " + what
        assert same(x, y), f"C buffer {i}: {int((x != y).sum())} elements differ from the per-item calls (NaN counted): " + what
    for P in (PA, PB):
        for x, h in zip(P.download(), P.host):
            assert gu.bits_equal(x, h), "an operand buffer was written: " + what
    if oracle_item is not None:
        b = oracle_item
        W = g.lib().gemmul8_batched_item_bytes(int(dt.kind == "c"), backend, m, n, k, N)
        v = gu.work_vectors(work, ol.DT[dt], backend, m, n, k, N, b * W)
        Co = np.asarray(ol.gemm(As[b], Bs[b], N, fastmode=fast, backend=backend, opA=opA, opB=opB, alpha=alpha, beta=beta, C0=C0s[b], sftA_in=v["sftA"], sftB_in=v["sftB"]))
        assert np.isfinite(Co).all()
        wb = PC.window(got, b)
        assert gu.bits_equal(wb, Co), f"item {b}: {int((wb != Co).sum())} entries differ from the oracle: " + what
    return PC, got


def data(dt, m, n, k, batch, opA="N", opB="N", seed=0):
    return gu.batched_data(dt, m, n, k, batch, opA, opB, rng=np.random.default_rng(seed))


SHUFFLE = [3, 0, 4, 1, 2]   # allocation order of the five items


@pytest.mark.parametrize("dtype,N", [(np.float64, 14), (np.float32, 7), (np.complex128, 15), (np.complex64, 8)])
@pytest.mark.parametrize("fast", [False, True])
def test_scattered_items_equal_per_item_calls_and_the_oracle(dtype, N, fast):
    As, Bs, C0s = data(dtype, 150, 70, 210, 5, seed=N + fast)
    ptr_case(As, Bs, C0s, N, fast, PA=place(As, separate=True, order=SHUFFLE), PB=place(Bs, separate=True, order=SHUFFLE[::-1]),
             PC=place(C0s, separate=True, c=True, order=SHUFFLE), oracle_item=3)


@pytest.mark.parametrize("dtype,N", [(np.float64, 12), (np.float32, 6), (np.complex128, 9), (np.complex64, 7)])
@pytest.mark.parametrize("fast", [False, True])
def test_fp8_backend_scattered_items(dtype, N, fast):
    As, Bs, C0s = data(dtype, 150, 70, 210, 5, seed=100 + N + fast)
    ptr_case(As, Bs, C0s, N, fast, backend=g.FP8, PA=place(As, separate=True, order=SHUFFLE), PB=place(Bs, separate=True, order=SHUFFLE[::-1]),
             PC=place(C0s, separate=True, c=True, order=SHUFFLE), oracle_item=1 if not fast else None)


@pytest.mark.parametrize("dtype,N", [(np.float64, 14), (np.complex128, 15)])
@pytest.mark.parametrize("opA", ["N", "T", "C"])
@pytest.mark.parametrize("opB", ["N", "T", "C"])
def test_ops(dtype, N, opA, opB):
    """{N, T, C}^2; 256^3 with batch 9: the items share workgroups of the persistent residue-GEMM kernel"""
    for m, n, k, batch in ((37, 41, 300, 3), (300, 530, 64, 2), (256, 256, 256, 9)):
        As, Bs, C0s = data(dtype, m, n, k, batch, opA, opB, seed=m + n + k)
        ptr_case(As, Bs, C0s, N, False, opA=opA, opB=opB)


@pytest.mark.parametrize("dtype,N", [(np.float64, 14), (np.float32, 7), (np.complex64, 8)])
@pytest.mark.parametrize("which", ["A", "B", "C"])
@pytest.mark.parametrize("odd_ld", [False, True])
@pytest.mark.parametrize("opA,opB", [("N", "N"), ("T", "T")])
def test_alignment_is_decided_per_item(dtype, N, which, odd_ld, opA, opB):
    """Items carved from one buffer: item 0 on a 16-byte boundary, items 1 and 2 one element behind one -- for one operand at a time.  The leading dimension is
    one per call: with an even one (whole 16-byte pieces per column) item 0 qualifies for every 16-byte form and item 1 for none; with an odd one item 2 is
    the item that is misaligned in base AND pitch, next to an item 0 whose base alone is aligned.  What the host could decide from item 0 is wrong for the others
    either way.  Both operand forms (row-strided and K-major)."""
    dt = np.dtype(dtype)
    m, n, k = 136, 72, 264   # multiples of 8: ld = rows is a whole number of 16-byte pieces for every type
    As, Bs, C0s = data(dt, m, n, k, 3, opA, opB, seed=5)
    pad = 1 if odd_ld else 0
    sh = [0, 1, 1]
    for fast in (False, True):
        ptr_case(As, Bs, C0s, N, fast, opA=opA, opB=opB, PA=place(As, pad if which == "A" else 0, sh if which == "A" else None),
                 PB=place(Bs, pad if which == "B" else 0, sh if which == "B" else None),
                 PC=place(C0s, pad if which == "C" else 0, sh if which == "C" else None, c=True), what=f"misaligned {which}")


@pytest.mark.parametrize("offset_c", [False, True])
@pytest.mark.parametrize("dtype", [np.float64, np.complex128])
def test_crt_form_at_the_shape_of_the_lds_dma_kernel(dtype, offset_c):
    """m x n = 1024 x 4096 (complex: 512 x 4096), small N: whole 1024-byte units per column and 4096 of them -- where the strided form selects the LDS-DMA CRT
    from C's address.  Item 1's C one element off a 16-byte boundary (real) / all items aligned: the same bits as the per-item calls (which do take
    the DMA form for an aligned C)."""
    dt = np.dtype(dtype)
    m, n, k, N = (1024 if dt.kind == "f" else 512), 4096, 64, 4
    As, Bs, C0s = data(dt, m, n, k, 2, seed=11)
    ptr_case(As, Bs, C0s, N, False, PC=place(C0s, 0, [0, 1] if offset_c else None, c=True), what="dma-shaped CRT")


def test_shared_operands():
    """every B entry the same pointer, two equal A entries"""
    As, Bs, C0s = data(np.float64, 150, 70, 210, 4, seed=3)
    As[2] = As[0]
    Bs = [Bs[0]] * 4
    PA, PB = place(As, separate=True), place(Bs, separate=True)
    assert len(set(PB.addrs())) == 1 and PA.addrs()[2] == PA.addrs()[0] and len(set(PA.addrs())) == 3
    for fast in (False, True):
        ptr_case(As, Bs, C0s, 14, fast, PA=PA, PB=PB)


@pytest.mark.parametrize("dtype,N,backend", [(np.float64, 14, g.INT8), (np.complex64, 8, g.INT8), (np.float32, 6, g.FP8)])
def test_guard_bytes_around_views(dtype, N, backend):
    """items are views with ld = rows + 7 inside larger buffers: every byte outside the C windows keeps its value (ptr_case checks it for every case; here
    with a pitch that is no multiple of anything)"""
    As, Bs, C0s = data(dtype, 150, 70, 210, 3, seed=8)
    PC, got = ptr_case(As, Bs, C0s, N, False, backend=backend, PA=place(As, 7, [1, 0, 3]), PB=place(Bs, 7, [0, 1, 1]), PC=place(C0s, 7, [1, 0, 1], c=True))
    assert sum(int(o.sum()) for o in PC.outside()) > 7 * 70 * 3


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("opA", ["N", "T"])
def test_tall_operand_where_a_single_call_takes_the_one_read_extract(batch, opA):
    """float64 accurate mode, m = 8192 rows, aligned: the per-item gemmul8_gemm calls take the one-read bound extract for a row-strided A, the pointer-array call
    (batch 1 included) must not decide that from an address it cannot read -- and gives the same bits"""
    As, Bs, C0s = data(np.float64, 8192, 64, 64, batch, opA, "N", seed=batch)
    ptr_case(As, Bs, C0s, 14, False, opA=opA)


def test_fp8_small_n_and_complex64():
    """n = 48: e4m3 byte planes instead of FP6 panel images; complex64 on FP8: the four-k-per-lane writer"""
    for dt, N in ((np.float32, 6), (np.float64, 12), (np.complex64, 7)):
        for n in (48, 70):
            As, Bs, C0s = data(dt, 150, n, 210, 3, seed=n)
            ptr_case(As, Bs, C0s, N, False, backend=g.FP8)


@pytest.mark.parametrize("dtype,N", [(np.float64, 14), (np.complex64, 8)])
@pytest.mark.parametrize("fast", [False, True])
def test_nonfinite_mode_1(dtype, N, fast):
    """a NaN in one row of A of item 2 only, an Inf in one column of B of item 0 only: every item equals its per-item call in mode 1 (ptr_case restores the
    mode in a finally)"""
    As, Bs, C0s = data(dtype, 150, 70, 210, 3, seed=2)
    As[2][17, 40] = np.nan
    Bs[0][100, 33] = np.inf
    before = g.set_nonfinite_mode(0)
    try:
        PC, got = ptr_case(As, Bs, C0s, N, fast, mode=1)
        assert g.set_nonfinite_mode(0) == 0   # restored
    finally:
        g.set_nonfinite_mode(before)
    w = [PC.window(got, b) for b in range(3)]
    assert np.isnan(w[2][17, :]).all() and not np.isnan(np.delete(w[2], 17, axis=0)).any()
    assert not np.isfinite(w[0][:, 33]).all() and np.isfinite(np.delete(w[0], 33, axis=1)).all()
    assert np.isfinite(w[1]).all()


def test_arrays_written_in_stream_order_right_before_the_call():
    """the arrays are filled by asynchronous copies on the call's stream, no synchronisation in between: the kernels read them in stream order"""
    dt = np.dtype(np.float64)
    m, n, k, N, batch = 150, 70, 210, 14, 4
    As, Bs, C0s = data(dt, m, n, k, batch, seed=6)
    PA, PB, PC = place(As, separate=True), place(Bs, separate=True), place(C0s, separate=True, c=True)
    PC1 = PC.twin()
    work = batch_work(dt, g.INT8, m, n, k, N, batch)
    alpha, beta = scalars(dt)
    pinned = [torch.tensor(P.addrs(), dtype=torch.int64).pin_memory() for P in (PA, PB, PC)]
    arrs = [torch.zeros(batch, dtype=torch.int64, device="cuda") for _ in range(3)]   # null entries until the copies land
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for a, p in zip(arrs, pinned):
            a.copy_(p, non_blocking=True)
        call_ptr(dt, g.INT8, "N", "N", m, n, k, alpha, beta, arrs[0], PA.ld, arrs[1], PB.ld, arrs[2], PC.ld, batch, N, False, work, stream=s.cuda_stream)
    s.synchronize()
    call_items(dt, g.INT8, "N", "N", m, n, k, alpha, beta, PA.addrs(), PA.ld, PB.addrs(), PB.ld, PC1.addrs(), PC1.ld, N, False)
    for x, y in zip(PC.download(), PC1.download()):
        assert gu.bits_equal(x, y)


def test_captured_call_reads_the_arrays_at_replay():
    """one call captured in a graph (linear: one stream, no parallel branches) after a warm-up; the CONTENTS of A_array are then overwritten with other valid
    pointers: the replay computes on the new items"""
    dt = np.dtype(np.float64)
    m, n, k, N, batch = 150, 70, 210, 14, 3
    As, Bs, C0s = data(dt, m, n, k, batch, seed=7)
    As2 = [np.asfortranarray(a[::-1, ::-1] * 3.0) for a in As]
    PA, PA2, PB, PC = place(As, separate=True), place(As2, separate=True), place(Bs, separate=True), place(C0s, separate=True, c=True)
    PC1 = PC.twin()
    work = batch_work(dt, g.INT8, m, n, k, N, batch)
    alpha, beta = scalars(dt)[0], 0.0   # beta = 0: the warm-up and the capture leave nothing behind in C that the replay reads
    arrA, arrB, arrC = dev_array(PA.addrs()), dev_array(PB.addrs()), dev_array(PC.addrs())
    args = (dt, g.INT8, "N", "N", m, n, k, alpha, beta, arrA, PA.ld, arrB, PB.ld, arrC, PC.ld, batch, N, False, work)
    call_ptr(*args)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call_ptr(*args)
    arrA.copy_(torch.tensor(PA2.addrs(), dtype=torch.int64))
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    call_items(dt, g.INT8, "N", "N", m, n, k, alpha, beta, PA2.addrs(), PA2.ld, PB.addrs(), PB.ld, PC1.addrs(), PC1.ld, N, False)
    for x, y in zip(PC.download(), PC1.download()):
        assert gu.bits_equal(x, y), "the replay did not compute on the pointers A_array held at replay"
    call_items(dt, g.INT8, "N", "N", m, n, k, alpha, beta, PA.addrs(), PA.ld, PB.addrs(), PB.ld, PC1.addrs(), PC1.ld, N, False)
    assert not any(gu.bits_equal(x, y) for x, y in zip(PC.download(), PC1.download()))   # (the old pointers give other results: the check above can tell)


def test_python_wrapper():
    """gemmul8_amd.gemm_batched_ptr on lists of views (Cs=None allocates) and on address tensors"""
    rng = np.random.default_rng(21)
    batch, m, n, k, N = 4, 130, 50, 96, 14
    bigA = torch.from_numpy(gu.rand_spread((batch, k, m + 3), np.float64, rng)).cuda()
    Avs = [bigA[b, :, 1:m + 1] for b in range(batch)]                        # views: ld = m + 3, one element off the row start
    Bt = torch.from_numpy(gu.rand_spread((n, k), np.float64, rng)).cuda()
    Bvs = [Bt] * batch                                                       # the same tensor repeated
    Cs, work = g.gemm_batched_ptr(Avs, Bvs, N)
    assert len(Cs) == batch and all(c.shape == (n, m) and c.dtype == torch.float64 for c in Cs)
    torch.cuda.synchronize()
    refs = []
    for b in range(batch):
        Ci, _, _ = g.gemm(Avs[b].contiguous(), Bt, N)
        refs.append(Ci)
        assert torch.equal(Cs[b].view(torch.uint8), Ci.view(torch.uint8)), b
    # transposed operands, given Cs with a leading dimension of their own, alpha / beta
    bigC = torch.from_numpy(gu.rand_spread((batch, n, m + 5), np.float64, rng)).cuda()
    C0 = bigC.clone()
    Cvs = [bigC[b, :, 2:m + 2] for b in range(batch)]
    At = [a.contiguous().T.contiguous() for a in Avs]                        # stored k x m -> m x k: op T
    out, _ = g.gemm_batched_ptr(At, Bvs, N, opA="T", alpha=-1.5, beta=0.5, Cs=Cvs, work=work)
    torch.cuda.synchronize()
    assert out[0] is Cvs[0]
    for b in range(batch):
        Ci = C0[b, :, 2:m + 2].contiguous()
        g.gemm(At[b], Bt, N, opA="T", alpha=-1.5, beta=0.5, C_out=Ci)
        assert torch.equal(Cvs[b].contiguous().view(torch.uint8), Ci.view(torch.uint8)), b
    outside = torch.ones_like(bigC, dtype=torch.bool)
    outside[:, :, 2:m + 2] = False
    assert torch.equal(bigC[outside].view(torch.uint8), C0[outside].view(torch.uint8))
    # address tensors
    pa = torch.tensor([a.data_ptr() for a in Avs], dtype=torch.int64).cuda()
    pb = torch.tensor([Bt.data_ptr()] * batch, dtype=torch.int64).cuda()
    C2 = [torch.zeros((n, m), dtype=torch.float64, device="cuda") for _ in range(batch)]
    pc = torch.tensor([c.data_ptr() for c in C2], dtype=torch.int64).cuda()
    ret, _ = g.gemm_batched_ptr(pa, pb, N, Cs=pc, m=m, n=n, k=k, lda=m + 3, ldb=k, ldc=m, dtype=torch.float64)
    torch.cuda.synchronize()
    assert ret is pc
    for b in range(batch):
        assert torch.equal(C2[b].view(torch.uint8), refs[b].view(torch.uint8)), b
    # a stream of the caller's that is not torch's current one: the wrapper's copies of the arrays are ordered on it, ahead of the kernels
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    Cside, _ = g.gemm_batched_ptr(Avs, Bvs, N, stream=side.cuda_stream)
    side.synchronize()
    for b in range(batch):
        assert torch.equal(Cside[b].view(torch.uint8), refs[b].view(torch.uint8)), b
    with pytest.raises(TypeError):
        g.gemm_batched_ptr(pa, pb, N, Cs=pc)                                 # address tensors without the shape
    with pytest.raises(TypeError):
        g.gemm_batched_ptr(Avs, [Bt.float()] * batch, N)                     # mixed dtypes
