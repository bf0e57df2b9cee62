"""examples/encrypted_compare.py runs end to end on the GPU: 32-bit a < b and a DFA match on encrypted 8-character
strings through CMUX graphs, their results combined by a gate, decrypt to the plaintext computation.  Its automaton
is checked on plain strings without a GPU."""
import importlib.util
import os

import pytest

from conftest import ROOT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_example_automaton_on_plain_strings():
    import tfhe_amd
    ex = _load("encrypted_compare")
    gr = tfhe_amd.CmuxGraph.dfa(3, ex.contains_ab_dfa(), {2}, 8, 8)
    assert gr.plan()[2] <= 64 and gr.n_nodes < 400
    for w in ex.WORDS + ["abababab", "bbbbbbba", "aaaaaaaa", "zzzzzzab"]:
        bits = [(ord(ch) >> j) & 1 for ch in w for j in range(8)]
        assert gr.evaluate_plain(bits) == [(int("ab" in w), 0)], w


@pytest.mark.gpu
def test_encrypted_compare_example(capsys):
    assert _load("encrypted_compare").main(["--pairs", "4"]) == 0
    out = capsys.readouterr().out
    assert "k_cmux_rot<3>" in out and "both:" in out and "Success" in out
