"""What of "encryption to shares" and the BFV slot map needs no GPU: the refusals of the five new entry points that come before the context is
looked at or that report its absence (as tests/test_capi_refusals_host.py pins them for the older calls), DeviceSampler.e2s_args, the host side
of mkbfv.SlotMap (constructors and apply) on a stand-in for the parameters."""
import ctypes as C

import numpy as np
import pytest

KEY = (C.c_uint32 * 8)(*range(1, 9))
ANON = "mkhe: null context"


def named(entry):
    return entry + ": null context"


# (entry, arguments behind the context, return code, message)
ROWS = [
    ("mkhe_e2s_share", (1, None, None, None, KEY, 1, -1, None, 1, None), 1, "mkhe_e2s_share: mask_bits must be 0 .. 120"),
    ("mkhe_e2s_share", (1, None, None, None, KEY, 1, 121, None, 1, None), 1, "mkhe_e2s_share: mask_bits must be 0 .. 120"),
    ("mkhe_e2s_share", (1, None, None, None, None, 1, 1, None, 1, None), 1, "mkhe_e2s_share: null key"),
    ("mkhe_e2s_share", (1, None, None, None, None, 1, 0, None, 1, None), 1, named("mkhe_e2s_share")),
    ("mkhe_e2s_share", (1, None, None, None, KEY, 1, 120, None, 1, None), 1, named("mkhe_e2s_share")),
    ("mkhe_e2s_merge", (1, None, 0, None, 1, None), 1, named("mkhe_e2s_merge")),
    ("mkhe_bfv_e2s_share", (1, None, None, None, KEY, 1, -1, None, None), 1, "mkhe_bfv_e2s_share: flood_bits must be 0 .. 1024"),
    ("mkhe_bfv_e2s_share", (1, None, None, None, KEY, 1, 1025, None, None), 1, "mkhe_bfv_e2s_share: flood_bits must be 0 .. 1024"),
    ("mkhe_bfv_e2s_share", (1, None, None, None, None, 1, 0, None, None), 1, "mkhe_bfv_e2s_share: null key"),
    ("mkhe_bfv_e2s_share", (1, None, None, None, KEY, 1, 0, None, None), 1, named("mkhe_bfv_e2s_share")),
    ("mkhe_bfv_slot_map_prepare", (None, None, None), 1, ANON),
    ("mkhe_bfv_slot_map", (1, None, None, None), 1, ANON),
]


@pytest.mark.parametrize("entry,args,rc,message", ROWS, ids=["%s-%d" % (r[0], i) for i, r in enumerate(ROWS)])
def test_a_call_without_a_context_is_refused_with_exactly_this_message(entry, args, rc, message):
    from mkhe_kklss_amd._abi import lib
    # a message of another call first, so that the one read back is this call's
    assert lib().mkhe_swk_fold(None, None, 0, 0) == 1 and lib().mkhe_last_error().decode() == "mkhe_swk_fold: null argument"
    assert getattr(lib(), entry)(None, *args) == rc
    assert lib().mkhe_last_error().decode() == message


def test_e2s_args_takes_one_value_of_the_shared_counter():
    from mkhe_kklss_amd import mkrlwe
    s = mkrlwe.DeviceSampler(key=bytes(range(32)), insecure_test_only=True)
    assert s.counter == 0
    key, nonce = s.e2s_args()
    assert nonce == 0 and s.counter == 1 and list(key) == list(s.encrypt_args()[0])
    assert s.counter == 2 and s.e2s_args()[1] == 2 and s.counter == 3
    # e2s_args then encrypt_args take the two values refresh_args takes
    a, b = (mkrlwe.DeviceSampler(key=bytes(range(32)), insecure_test_only=True) for _ in range(2))
    _, mask, enc = a.refresh_args()
    assert (b.e2s_args()[1], b.encrypt_args()[1]) == (mask, enc) and a.counter == b.counter == 2


class Stub:
    """what mkbfv.SlotMap reads of the parameters on the host"""

    def __init__(self, N, T):
        self._N, self._T = N, T

    def N(self):
        return self._N

    def T(self):
        return self._T


def test_slot_map_apply_on_eight_slots_by_hand():
    from mkhe_kklss_amd import mkbfv
    p = Stub(8, 17)
    m = mkbfv.SlotMap(p, [1, 2, 3, 0, 5, 6, 7, 4], [1, 2, 3, 4, 16, 0, -1, 18])
    assert m.mult.tolist() == [1, 2, 3, 4, 16, 0, 16, 1]                                  # taken mod T
    #                 slots   1  2  3  4  5  6  7  8
    # gathered                2  3  4  1  6  7  8  5
    # times mult              2  6 12  4 96  0 128 5   mod 17 = 2 6 12 4 11 0 9 5, centred in (-8, 8]
    assert m.apply([1, 2, 3, 4, 5, 6, 7, 8]).tolist() == [2, 6, -5, 4, -6, 0, -8, 5]
    assert m.apply([[1, 2, 3, 4, 5, 6, 7, 8], [-1, 0, 0, 0, 0, 0, 0, 17]]).tolist() == [[2, 6, -5, 4, -6, 0, -8, 5], [0, 0, 0, -4, 0, 0, 0, 0]]
    ident = mkbfv.SlotMap(p, np.arange(8))
    assert ident.apply([9, -9, 16, 17, 18, 0, 8, -8]).tolist() == [-8, 8, -1, 0, 1, 0, 8, -8]
    # a rotation by k moves slot i + k to slot i within each row of N/2; swap_rows exchanges the rows
    v = [10, 11, 12, 13, 20, 21, 22, 23]
    assert mkbfv.SlotMap.Rotation(Stub(8, 97), 1).apply(v).tolist() == [11, 12, 13, 10, 21, 22, 23, 20]
    assert mkbfv.SlotMap.Rotation(Stub(8, 97), 5, swap_rows=True).apply(v).tolist() == [21, 22, 23, 20, 11, 12, 13, 10]
    assert mkbfv.SlotMap.Rotation(Stub(8, 97), -1).apply(v).tolist() == [13, 10, 11, 12, 23, 20, 21, 22]
    assert mkbfv.SlotMap.Permutation(Stub(8, 97), [7, 6, 5, 4, 3, 2, 1, 0]).apply(v).tolist() == v[::-1]
    assert mkbfv.SlotMap(Stub(8, 97), [0] * 8).apply(v).tolist() == [10] * 8              # a replicating index is no permutation and is a map


def test_slot_map_constructors_refuse_wrong_shapes_and_indices():
    from mkhe_kklss_amd import mkbfv
    from mkhe_kklss_amd._abi import MkheError
    p = Stub(8, 17)
    for index, mult in (([0] * 7, None), ([0] * 9, None), ([[0] * 8], None), ([0.0] * 8, None), ([0] * 7 + [8], None), ([-1] + [0] * 7, None),
                        ([0] * 8, [1] * 7), ([0] * 8, [1.5] * 8), ([0] * 8, [[1] * 8])):
        with pytest.raises(MkheError, match="mkbfv.SlotMap"):
            mkbfv.SlotMap(p, index, mult)
    for perm in ([0] * 8, [0, 1, 2, 3, 4, 5, 6, 8], [0, 1, 2]):
        with pytest.raises(MkheError, match="Permutation"):
            mkbfv.SlotMap.Permutation(p, perm)
    with pytest.raises(MkheError, match="expected 8 slots"):
        mkbfv.SlotMap(p, np.arange(8)).apply([1, 2, 3])
