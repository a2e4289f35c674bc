"""Compile-time properties of gemm_i8_sbs_kernel (csrc/oz2_gemm_i8.hip: the ping-pong residue GEMM with the wave halves' epilogues side by side), read from
the code object's metadata the way tests/test_kernel_resources.py and tools/kernel_regs.py do: one instantiation, 168 registers (three waves per SIMD),
no scratch at all -- a value kept live across the moved barrier must not be spilled: its reload would wait for the previous tile's stores --, and no
vector-memory wait in the blocks that hold the K loop's MFMAs.  No GPU needed; about 40 s of compilation."""
import re

import pytest

import test_kernel_resources as kr

pytestmark = kr.pytestmark


@pytest.fixture(scope="module")
def sbs():
    return {n: v for n, v in kr._kernels(kr._asm("oz2_gemm_i8.hip")).items() if "gemm_i8_sbs_kernel" in n}


def test_one_instantiation_168_registers_no_scratch(sbs):
    assert len(sbs) == 1, sorted(sbs)                                  # <EPI_MOD, KBAR = false, FUSE = 0, SMALLK = false>: the only launch
    (name, (vg, sc, blocks)), = sbs.items()
    assert "ILi0ELb0ELi0ELb0E" in name, name
    assert vg <= 168, vg
    assert sc == 0, sc
    loops = [b for b in blocks if any("v_mfma" in l for l in b)]
    assert sum(sum("v_mfma" in l for l in b) for b in loops) == 128, "the K loop's K-step and the lagging half's peeled last one: four segments of 16 MFMAs each"
    for b in loops:
        assert not any(re.match(r"s_waitcnt vmcnt", l) for l in b), "vmcnt wait in an MFMA block"
