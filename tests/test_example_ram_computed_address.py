"""examples/encrypted_ram_computed_address.py: its circuit reads the input wires as a select node's entries, and on
the GPU every read decrypts to the addressed word."""
import importlib.util
import os

import pytest

from conftest import ROOT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_examples_circuit_reads_the_table_wires_at_depth_3():
    c = _load("encrypted_ram_computed_address").build_circuit(2)
    levels, depth = c.schedule()
    assert depth == 3 and c.n_inputs == 16 + 4 and len(c.nodes) == 2 * 18
    reads = [s for s in c.sel if s is not None and s == list(range(16))]
    assert len(reads) == 2 and levels.tolist().count(3) == 2


@pytest.mark.gpu
def test_encrypted_ram_computed_address_example():
    assert _load("encrypted_ram_computed_address").main(["--reads", "3"]) == 0
