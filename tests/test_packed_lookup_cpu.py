"""CPU tests of the packed lookup's host-only half: tfhe_packed_lookup_plan against a Python
restatement, tfhe_lookup_table_pack_slots against numpy and against tfhe_lookup_table_pack_bits
where an entry fills a TRLWE, and the entries' checks that return before a device is touched."""
import ctypes as C

import numpy as np
import pytest

import tfhe_amd

u32p = C.POINTER(C.c_uint32)
PLUS, MINUS = 0x20000000, 0xE0000000  # f64ToTorus(+-0.125)


def plan_by_hand(N, k, width):
    """stride = the next power of two >= width, slots = N / stride, h = min(k, log2 slots), v = k - h;
    None where v > 12 (the tree's limit)."""
    stride = 1
    while stride < width:
        stride *= 2
    slots = N // stride
    h = min(k, slots.bit_length() - 1)
    v = k - h
    if v > 12:
        return None
    return dict(stride=stride, slots=slots, h=h, v=v, trlwes=1 << v, cmuxes=(1 << v) - 1 + h,
                rot=[2 * N - stride * (1 << j) if j < h else 0 for j in range(10)])


@pytest.mark.parametrize("width", [1, 3, 8, 64, 1024])
@pytest.mark.parametrize("k", [1, 5, 7, 8, 22])
def test_plan_matches_restatement(k, width):
    p = tfhe_amd.make_params("128")
    want = plan_by_hand(p.N, k, width)
    if want is None:
        assert k - min(k, (p.N // width).bit_length() - 1) > 12
        with pytest.raises(tfhe_amd.TfheError) as err:
            tfhe_amd.packed_lookup_plan(p, k, width)
        assert err.value.status == tfhe_amd.ERR_INVALID
        return
    got = tfhe_amd.packed_lookup_plan(p, k, width)
    assert {f: getattr(got, f) for f in ("stride", "slots", "h", "v", "trlwes", "cmuxes")} == \
        {f: want[f] for f in ("stride", "slots", "h", "v", "trlwes", "cmuxes")}
    assert list(got.rot) == want["rot"]


def test_plan_shapes_of_the_sbox_and_the_largest_table():
    p = tfhe_amd.make_params("128")
    sbox = tfhe_amd.packed_lookup_plan(p, 8, 8)
    assert (sbox.trlwes, sbox.h, sbox.v, sbox.cmuxes) == (2, 7, 1, 8)
    assert list(sbox.rot[:7]) == [2048 - 8 * (1 << j) for j in range(7)]
    big = tfhe_amd.packed_lookup_plan(p, 22, 1)  # 4,096 x 1,024 one-bit entries
    assert (big.h, big.v, big.trlwes) == (10, 12, 4096)
    # the refused ones are among the parametrised cases: k = 22 at widths 3 .. 1024
    assert plan_by_hand(p.N, 22, 3) is None and plan_by_hand(p.N, 22, 1) is not None


def test_plan_rejects_bad_arguments():
    lib = tfhe_amd.load_library()
    p = tfhe_amd.make_params("128")
    out = tfhe_amd.PackedPlan()
    INV = tfhe_amd.ERR_INVALID
    assert lib.tfhe_packed_lookup_plan(None, 8, 8, C.byref(out)) == INV
    assert lib.tfhe_packed_lookup_plan(C.byref(p), 8, 8, None) == INV
    assert lib.tfhe_packed_lookup_plan(C.byref(p), 0, 8, C.byref(out)) == INV
    assert lib.tfhe_packed_lookup_plan(C.byref(p), 8, 0, C.byref(out)) == INV
    assert lib.tfhe_packed_lookup_plan(C.byref(p), 8, p.N + 1, C.byref(out)) == INV
    assert lib.tfhe_packed_lookup_plan(C.byref(p), 13, p.N, C.byref(out)) == INV
    assert lib.tfhe_packed_lookup_plan(C.byref(p), 12, p.N, C.byref(out)) == 0
    p.N = 512
    assert lib.tfhe_packed_lookup_plan(C.byref(p), 8, 8, C.byref(out)) == INV


@pytest.mark.parametrize("pname", ["128", "uint4"])
@pytest.mark.parametrize("k,width", [(1, 1), (5, 8), (8, 8), (7, 3), (3, 64), (11, 1), (4, 33)])
def test_pack_slots_matches_numpy(pname, k, width):
    p = tfhe_amd.make_params(pname)
    N = p.N
    plan = plan_by_hand(N, k, width)
    values = np.random.default_rng(100 * k + width).integers(0, 1 << 63, 1 << k, dtype=np.uint64) * 2 + 1
    got = tfhe_amd.lookup_table_pack_slots(p, values, width)
    assert got.shape == (plan["trlwes"], 2 * N)
    assert not got[:, :N].any()  # a = 0
    want = np.zeros((plan["trlwes"], N), np.uint32)
    e = np.arange(1 << k)
    for c in range(width):
        bit = ((values >> np.uint64(c)) & np.uint64(1)).astype(bool)
        want[e >> plan["h"], (e & ((1 << plan["h"]) - 1)) * plan["stride"] + c] = np.where(bit, PLUS, MINUS)
    assert np.array_equal(got[:, N:], want)
    # every coefficient outside an entry's width bits is 0: exactly 2^k * width words are set
    assert np.count_nonzero(got) == (1 << k) * width


def test_pack_slots_with_one_entry_per_trlwe_is_pack_bits():
    """width 33 .. 64 at N = 1024 gives stride 64, 16 slots; a stride of N (one entry per TRLWE, h = 0) needs
    width > N / 2, past pack_slots' 64 bits, so the degenerate layout is checked on the plan, and pack_slots
    against pack_bits entry by entry: slot s of TRLWE t holds what pack_bits puts at coefficient 0 of entry e."""
    p = tfhe_amd.make_params("128")
    N = p.N
    one = tfhe_amd.packed_lookup_plan(p, 3, N)
    assert (one.stride, one.slots, one.h, one.v, one.trlwes, one.cmuxes) == (N, 1, 0, 3, 8, 7)  # the CMUX tree alone
    for width in (1, 8, 64):
        k = 6
        plan = tfhe_amd.packed_lookup_plan(p, k, width)
        values = np.random.default_rng(width).integers(0, 1 << 63, 1 << k, dtype=np.uint64) * 2 + 1
        slots = tfhe_amd.lookup_table_pack_slots(p, values, width)
        bits = tfhe_amd.lookup_table_pack_bits(p, values, width)
        for e in range(1 << k):
            at = N + (e & ((1 << plan.h) - 1)) * plan.stride
            assert np.array_equal(slots[e >> plan.h, at:at + width], bits[e, N:N + width]), (width, e)


def test_pack_slots_rejects_bad_arguments():
    lib = tfhe_amd.load_library()
    p = tfhe_amd.make_params("128")
    v = np.ones(256, np.uint64)
    vp_ = v.ctypes.data_as(C.POINTER(C.c_uint64))
    t = np.zeros(2 * 2 * p.N, np.uint32)
    tp = t.ctypes.data_as(u32p)
    INV = tfhe_amd.ERR_INVALID
    assert lib.tfhe_lookup_table_pack_slots(None, vp_, 8, 8, tp) == INV
    assert lib.tfhe_lookup_table_pack_slots(C.byref(p), None, 8, 8, tp) == INV
    assert lib.tfhe_lookup_table_pack_slots(C.byref(p), vp_, 8, 8, None) == INV
    assert lib.tfhe_lookup_table_pack_slots(C.byref(p), vp_, 8, 65, tp) == INV
    assert lib.tfhe_lookup_table_pack_slots(C.byref(p), vp_, 8, 0, tp) == INV
    assert lib.tfhe_lookup_table_pack_slots(C.byref(p), vp_, 0, 8, tp) == INV
    assert lib.tfhe_lookup_table_pack_slots(C.byref(p), vp_, 8, 8, tp) == 0
    with pytest.raises(ValueError):
        tfhe_amd.lookup_table_pack_slots(p, [1, 2, 3], 8)


def test_entries_refuse_a_null_context_and_are_exported():
    lib = tfhe_amd.load_library()
    x = np.zeros(2048, np.uint32)
    xp = x.ctypes.data_as(u32p)
    INV = tfhe_amd.ERR_INVALID
    assert lib.tfhe_gpu_rotate_by_bits_batch(None, None, xp, xp, 1, xp, xp, 1) == INV
    assert lib.tfhe_gpu_rotate_by_bits_dev(None, None, xp, xp, 1, None, None, 1) == INV
    assert lib.tfhe_gpu_packed_lookup_batch(None, None, xp, 3, 8, xp, xp, 1) == INV
    assert lib.tfhe_gpu_packed_lookup_dev(None, None, xp, 3, 8, None, None, 1) == INV
    for name in ("tfhe_gpu_rotate_by_bits_batch", "tfhe_gpu_rotate_by_bits_dev", "tfhe_packed_lookup_plan",
                 "tfhe_lookup_table_pack_slots", "tfhe_gpu_packed_lookup_batch", "tfhe_gpu_packed_lookup_dev"):
        assert name in tfhe_amd.EXPORTED_SYMBOLS
