"""examples/encrypted_sbox_circuit.py: its circuit has the shape it describes, and on the GPU S[x ^ k] decrypts."""
import importlib.util
import os

import pytest

from conftest import ROOT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_examples_circuit_has_depth_4_and_four_select_nodes_per_byte():
    ex = _load("encrypted_sbox_circuit")
    box = ex.aes_sbox()
    assert sorted(box) == list(range(256)) and [box[v] for v in (0x00, 0x53, 0xFF)] == [0x63, 0xED, 0x16]
    c = ex.build_circuit(3)
    levels, depth = c.schedule()
    assert depth == 4 and len(c.nodes) == 3 * 4 * 17 and sum(s is not None for s in c.sel) == 12
    assert sorted(set(levels.tolist())) == [1, 2, 3, 4] and len(c.outputs) == 6


@pytest.mark.gpu
def test_encrypted_sbox_circuit_example():
    assert _load("encrypted_sbox_circuit").main(["--bytes", "3"]) == 0
