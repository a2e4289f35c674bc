"""CPU tests of gemmul8_set_nonfinite_mode (include/gemmul8_c.h): exported, declared, round-trips 0 -> 1 -> 0, returns the previous mode
and rejects anything but 0 and 1 -- through the C ABI and through gemmul8_amd.set_nonfinite_mode."""
import os
import re

import pytest

import gemmul8_amd as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -2  # GEMMUL8_E_ARG


@pytest.fixture
def lib():
    L = g.lib()
    L.gemmul8_set_nonfinite_mode(0)
    yield L
    L.gemmul8_set_nonfinite_mode(0)   # process-wide: leave the default behind


def test_setter_is_declared_exported_and_bound(lib):
    hdr = open(os.path.join(ROOT, "include", "gemmul8_c.h")).read()
    assert re.search(r"GEMMUL8_API\s+int\s+gemmul8_set_nonfinite_mode\s*\(\s*int\s+mode\s*\)", hdr)
    assert hasattr(lib, "gemmul8_set_nonfinite_mode")
    assert "gemmul8_set_nonfinite_mode" in g.EXPORTS


def test_round_trip_returns_previous_mode(lib):
    assert lib.gemmul8_set_nonfinite_mode(1) == 0
    assert lib.gemmul8_set_nonfinite_mode(1) == 1
    assert lib.gemmul8_set_nonfinite_mode(0) == 1
    assert lib.gemmul8_set_nonfinite_mode(0) == 0


@pytest.mark.parametrize("bad", [2, -1, 7])
def test_rejects_other_modes_and_keeps_the_current_one(lib, bad):
    assert lib.gemmul8_set_nonfinite_mode(1) == 0
    assert lib.gemmul8_set_nonfinite_mode(bad) == E_ARG
    assert lib.gemmul8_set_nonfinite_mode(0) == 1   # the rejected call changed nothing


def test_python_wrapper(lib):
    assert g.set_nonfinite_mode(g.NONFINITE_IEEE) == g.NONFINITE_REFERENCE
    with pytest.raises(ValueError):
        g.set_nonfinite_mode(2)
    assert g.set_nonfinite_mode(0) == 1
