"""examples/encrypted_computed_table.py runs end to end on the GPU: a table computed by 64 gates, packed by the
packing key switch and looked up by encrypted addresses decrypts to value[addr] ^ mask."""
import importlib.util
import os

import pytest

from conftest import ROOT


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "examples", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_encrypted_computed_table_example(capsys):
    assert _load("encrypted_computed_table").main(["--queries", "3"]) == 0
    out = capsys.readouterr().out
    assert "k_key_switch_gemm<8,2> + k_pack_rotate_acc" in out and "Success" in out
