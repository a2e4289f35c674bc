"""Host model of the workgroup barriers of the persistent INT8 residue GEMM in its ping-pong schedule (csrc/oz2_gemm_i8_kernel.inc, the branch without
KBAR; the producers' loop: csrc/oz2_gemm_i8_producer.inc and the kernel's producer branch), for gemm_i8_kernel's order and for gemm_i8_sbs_kernel's, in
which the lagging wave half takes the last barrier of a tile behind its epilogue.  No GPU, no compiler: every role is written down as the sequence of
what it does between its barriers, following the kernel text loop for loop, and the sequences are then held against each other:

  * every role arrives at the same number of barriers (a mismatch is a hang);
  * between two barriers at most one wave half is in an MFMA segment (the anti-phase the schedule is built on);
  * no ring slot is refilled before the last read of the panel it held (WAR), and no panel is read before the producers' wait for it (RAW).

Operand panel h = 2 g + isB of K-step g (counted across the workgroup's tiles) lives in ring slot h % 5."""
import pytest

TILES = (1, 2, 3)
KSTEPS = (2, 42)


def producer(is_b, tiles, kt):
    """One producer wave: A panels two K-steps ahead, B panels one K-step ahead; eight barriers per K-step.  (The same text serves both kernels.)"""
    total = tiles * kt                                    # K-steps of the workgroup = panels per operand
    ev = []
    nxt = 0                                               # PRODUCER_FETCH / PRODUCER_ADVANCE: the K-step of the panel fetched next; more = nxt < total

    def fetch():
        nonlocal nxt
        ev.append(("fill", 2 * nxt + is_b))
        nxt += 1
    fetch()                                               # panel 0
    ahead = False
    if not is_b and nxt < total:
        fetch()                                           # A(1)
        ahead = True
    ev.append(("landed", nxt - (2 if ahead else 1)))      # vmcnt(16) leaves the panel just issued in flight, vmcnt(0) nothing
    ev.append(("bar",))
    for g in range(total):                                # for vb ... for kt ...
        issued = nxt < total
        for sl in range(8):
            if issued and (not is_b or sl < 4):           # 2 DMA instructions in every slot (A) / 4 in slots 0-3 (B): the panel is being written from here on
                ev.append(("fill", 2 * nxt + is_b))
            if sl == 7:
                if issued:
                    nxt += 1
                # A after an issue: everything but the 16 instructions just issued; otherwise everything
                ev.append(("landed", nxt - (2 if (issued and not is_b) else 1)))
            ev.append(("bar",))
    ev.append(("bar",))
    return ev


def consumer(wm, tiles, kt, sbs, drop_last_deferred=False):
    """One consumer wave of half wm.  sbs: gemm_i8_sbs_kernel's order."""
    ev = [("bar",)]                                       # K-tile 0 published by the producers
    if wm == 1:
        ev.append(("bar",))                               # trailing half: one segment behind
    g = 0
    for tile in range(tiles):
        ev.append(("init", tile))
        if sbs and wm == 1 and tile != 0:
            ev.append(("bar",))                           # the previous tile's last barrier
        def kstep(defer):                                 # csrc/oz2_gemm_i8_pp_kstep.inc
            nonlocal g
            for ks2 in range(2):
                for ah in range(2):
                    if ah == 0:
                        ev.append(("read", 2 * g + 1))    # B fragments of the K half
                    ev.append(("read", 2 * g))            # A fragments of 64 rows
                    ev.append(("bar",))
                    ev.append(("mfma", g, 2 * ks2 + ah))
                    if not (defer and ks2 == 1 and ah == 1):
                        ev.append(("bar",))
            g += 1
        for k in range(kt - wm if sbs else kt):
            kstep(False)
        if sbs and wm == 1:
            kstep(True)                                   # the lagging half's last K-step of the tile, peeled
        ev.append(("epi", tile))
    if sbs and wm == 1 and tiles > 0 and not drop_last_deferred:
        ev.append(("bar",))                               # the last tile's last barrier
    if wm == 0:
        ev.append(("bar",))
    return ev


def intervals(ev):
    """[[events between barrier i - 1 and barrier i] for i = 0 .. number of barriers] (the last entry: behind the last barrier)"""
    out = [[]]
    for e in ev:
        if e[0] == "bar":
            out.append([])
        else:
            out[-1].append(e)
    return out


def roles(tiles, kt, sbs, **kw):
    r = {"producer A 0": producer(0, tiles, kt), "producer A 1": producer(0, tiles, kt), "producer B 0": producer(1, tiles, kt), "producer B 1": producer(1, tiles, kt),
         "half 0": consumer(0, tiles, kt, sbs), "half 1": consumer(1, tiles, kt, sbs, **kw)}
    return {name: intervals(ev) for name, ev in r.items()}


def check(rs, tiles, kt):
    counts = {name: len(iv) - 1 for name, iv in rs.items()}
    assert len(set(counts.values())) == 1, counts                                    # a hang otherwise
    nbar = counts["half 0"]
    assert nbar == 8 * tiles * kt + 2, nbar                                          # ... and the count the kernels have always had
    for i in range(nbar + 1):
        busy = [h for h in ("half 0", "half 1") if any(e[0] == "mfma" for e in rs[h][i])]
        assert len(busy) <= 1, (i, busy)
    # every half runs all its segments, in order
    for h in ("half 0", "half 1"):
        segs = [e[1:] for iv in rs[h] for e in iv if e[0] == "mfma"]
        assert segs == [(g, s) for g in range(tiles * kt) for s in range(4)], h
    last_read, first_read, first_fill, landed = {}, {}, {}, {}
    for name, iv in rs.items():
        for i, evs in enumerate(iv):
            for e in evs:
                if e[0] == "read":
                    last_read[e[1]] = max(last_read.get(e[1], -1), i)
                    first_read[e[1]] = min(first_read.get(e[1], 1 << 30), i)
                elif e[0] == "fill":
                    first_fill[e[1]] = min(first_fill.get(e[1], 1 << 30), i)
                elif e[0] == "landed":                                               # panels up to K-step e[1] of this producer's operand
                    is_b = "B" in name
                    for g in range(e[1] + 1):
                        landed.setdefault((2 * g + is_b, name), i)
    panels = range(2 * tiles * kt)
    assert sorted(first_fill) == list(panels) and sorted(last_read) == list(panels)  # every panel is fetched once per producer pair and read
    for h in panels:
        if h >= 5:
            assert last_read[h - 5] < first_fill[h], ("WAR", h, last_read[h - 5], first_fill[h])
        waits = [i for (p, _), i in landed.items() if p == h]
        assert len(waits) == 2 and max(waits) < first_read[h], ("RAW", h, waits, first_read[h])   # both waves of the pair waited, in an earlier interval


@pytest.mark.parametrize("kt", KSTEPS)
@pytest.mark.parametrize("tiles", TILES)
@pytest.mark.parametrize("sbs", [False, True], ids=["serial", "side-by-side"])
def test_barrier_counts_antiphase_and_ring_rules(sbs, tiles, kt):
    check(roles(tiles, kt, sbs), tiles, kt)


@pytest.mark.parametrize("kt", KSTEPS)
@pytest.mark.parametrize("tiles", TILES)
def test_where_the_epilogues_run(tiles, kt):
    """gemm_i8_kernel: the lagging half's epilogue of a tile one barrier interval behind the leading half's.  gemm_i8_sbs_kernel: in the same interval, together
    with the next tile's initialisation, and everything else of both halves in the interval it had."""
    def where(rs, h, what):
        return {e[1:]: i for i, evs in enumerate(rs[h]) for e in evs if e[0] == what}
    old, new = roles(tiles, kt, False), roles(tiles, kt, True)
    for t in range(tiles):
        assert where(old, "half 1", "epi")[(t,)] == where(old, "half 0", "epi")[(t,)] + 1
        assert where(new, "half 1", "epi")[(t,)] == where(new, "half 0", "epi")[(t,)] == where(old, "half 0", "epi")[(t,)]
        if t:
            assert where(new, "half 1", "init")[(t,)] == where(new, "half 0", "init")[(t,)]
    for h in ("half 0", "half 1"):
        for what in ("mfma", "read"):
            assert [[e for e in evs if e[0] == what] for evs in old[h]] == [[e for e in evs if e[0] == what] for evs in new[h]], (h, what)
    for name in old:
        if name.startswith("producer"):
            assert old[name] == new[name]


def test_the_model_sees_a_missing_barrier():
    """a deferred barrier that is never made up for is a count mismatch -- what this model exists to catch"""
    with pytest.raises(AssertionError):
        check(roles(2, 2, True, drop_last_deferred=True), 2, 2)
