"""examples/encrypted_table_64.py: its circuit is one level of extended select nodes over the 64 input wires, the
planned reads cover all 64 addresses without a carry, and on the GPU every read decrypts to the stored word."""
import importlib.util
import os

import pytest

from conftest import ROOT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_examples_circuit_is_one_level_of_extended_select_nodes():
    ex = _load("encrypted_table_64")
    c = ex.build_circuit(3)
    levels, depth, groups = c.schedule_ext()
    assert depth == 1 and groups.tolist() == [[0, 0, 3]] and c.n_inputs == 64 + 6 and len(c.nodes) == 3
    assert c.eta == [2, 2, 2] and all(s == list(range(64)) for s in c.sel) and c.m == 64
    assert [n[1] for n in c.nodes] == [[(64, 1), (65, 1)], [(66, 1), (67, 1)], [(68, 1), (69, 1)]]


@pytest.mark.parametrize("offsets", [[0, 5, 21], [63], [7, 40]])
def test_the_planned_reads_cover_every_address_without_a_carry(offsets):
    base, off = _load("encrypted_table_64").plan_reads(offsets)
    assert (base + off).tolist() == list(range(64)) and int(base.min()) >= 0 and int((base + off).max()) < 64
    assert int(off.max()) > 0


@pytest.mark.gpu
def test_encrypted_table_64_example():
    """64 reads, one per address (5.2 sigma per output at m = 64 with fresh inputs)."""
    assert _load("encrypted_table_64").main(["--offsets", "0", "5", "21"]) == 0
