"""CPU check of the schedule of ntt16_f2_kernel (csrc/engine_mulrelin.hip f2_build_schedule through mkhe_f2_schedule_probe): for every shape the engine
may ask for, every pass (party, limb slot, half limb, digit) is dealt to exactly one workgroup, the runs of a group are numbered 0, 1, .. in digit order,
the group's last run zeroes exactly the parts the group does not have, and no workgroup carries more runs than the kernel walks.  No GPU involved.
Replaces nothing in the reference: the loop order of mkrlwe/keyswitch_hoisted.go:161-178 is free (canonical sums)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from mkhe_kklss_amd._abi import lib

F2_SEGS = 3


VI_SUMS, VI_MAX, F2_PARTS_MAX = 13, 4, 11


def _max_parts(parties):
    """csrc/ntt_kernels.h f2_max_parts: members of out_0 x parts + the tensor term, and a party's own slot: parts + step E + tensor, within VI_SUMS summands"""
    return min((VI_SUMS - 1) // min(parties, VI_MAX), VI_SUMS - 2, F2_PARTS_MAX)


def _probe(parties, nb, nslots, weights, grid):
    """grid > 0: the cut on exactly that grid; grid < 0: the engine's plan for a device of -grid CUs"""
    w = (C.c_long * nslots)(*weights)
    segs = (C.c_ubyte * (abs(grid) * F2_SEGS * 8))()
    parts = C.c_int(0)
    nwg = lib().mkhe_f2_schedule_probe(parties, nb, nslots, w, grid, segs, C.byref(parts))
    return nwg, parts.value, np.frombuffer(segs, dtype=np.uint8).reshape(abs(grid), F2_SEGS, 8)


def _check(parties, nb, nslots, weights, grid):
    nwg, parts, segs = _probe(parties, nb, nslots, weights, grid)
    if nwg == 0:
        return 0
    planned, grid = grid < 0, abs(grid)
    assert 1 <= nwg <= grid and 1 <= parts <= _max_parts(parties)
    seen = np.zeros((parties, nslots, 2, nb), dtype=np.int32)
    runs = {}
    for wg in range(grid):
        for si in range(F2_SEGS):
            party, slot, half, d0, nd, part, pad0, pad1 = (int(x) for x in segs[wg, si])
            if nd == 0:
                continue
            assert wg < nwg and party < parties and slot < nslots and half < 2 and d0 + nd <= nb and pad1 == 0
            seen[party, slot, half, d0:d0 + nd] += 1
            runs.setdefault((party, slot, half), []).append((d0, nd, part, pad0))
    assert (seen == 1).all(), "a pass dealt %s times" % sorted(set(seen.flatten().tolist()))
    for g, rs in runs.items():
        rs.sort()
        assert [r[2] for r in rs] == list(range(len(rs))), (g, rs)            # parts in digit order
        assert all(r[3] == 0 for r in rs[:-1]) and rs[-1][3] == parts - len(rs), (g, rs, parts)
        assert len(rs) <= parts
    # the weighted load of the heaviest workgroup stays within one pass of the mean (the cut is by the midpoint of a pass's weight interval)
    load = np.zeros(grid)
    for wg in range(grid):
        for si in range(F2_SEGS):
            party, slot, half, d0, nd = (int(x) for x in segs[wg, si][:5])
            load[wg] += nd * weights[slot]
    total = sum(weights[s] for s in range(nslots)) * 2 * parties * nb
    assert load.max() <= total / (nwg if planned else grid) + max(weights) + 1e-9
    return parts


def test_headline_shape_is_two_even_parts():
    # PN15QP880, 4 parties, 14 digits, 16 limb slots, 256 workgroups, every pass the same cost: two runs of seven digits per group
    nwg, parts, segs = _probe(4, 14, 16, [100] * 16, 256)
    assert nwg == 256 and parts == 2
    assert (segs[:, 0, 4] == 7).all() and (segs[:, 1:, 4] == 0).all()
    _check(4, 14, 16, [100] * 16, 256)


@pytest.mark.parametrize("parties", [1, 2, 3, 4, 5, 6, 7, 8, 12, 16])
@pytest.mark.parametrize("level", [0, 1, 5, 9, 13])
def test_every_pass_exactly_once(parties, level):
    nb, nslots = level + 1, level + 1 + 2
    for grid in (256, 304, 64):
        _check(parties, nb, nslots, [100] * nslots, grid)
        w = [100] * nslots
        w[0] = 115
        w[-1] = w[-2] = 105
        _check(parties, nb, nslots, w, grid)


@pytest.mark.parametrize("parties", range(9, 17))
def test_every_pass_exactly_once_nine_to_sixteen_parties(parties):
    # the band in which out_0 has more members than one inverse job takes (VI_MAX = 4: parts <= 3), at EVERY level of PN15QP880 (14 Q + 2 P primes):
    # the cut on the whole chip (256 and 304 workgroups, a quarter of one) and the engine's plan for those chips
    for level in range(14):
        nb, nslots = level + 1, level + 1 + 2
        assert _max_parts(parties) == 3
        for grid in (256, 304, 64, -256, -304):
            _check(parties, nb, nslots, [100] * nslots, grid)
        w = [100] * nslots
        w[0] = 115
        w[-1] = w[-2] = 105
        _check(parties, nb, nslots, w, 256)
        _check(parties, nb, nslots, w, -256)


EXT_MAX_ITEMS, NTT_MAX_SLOTS = 64, 48      # csrc/poly_kernels.h, csrc/ntt_kernels.h


def _tail_jobs(ids0, ids1, parts, members):
    """The tail batch of a MulAndRelin whose F2 products arrive in `parts` parts, restated from csrc/engine_mulrelin.hip (mr_finish_tail: per party of
    op0 the products with v_i -> out_0 and with u -> its own slot, then step E per party of op1 -> its slot; the tensor term rides on the first product
    of every destination) and csrc/engine.hip (ext_plan_merge: the products of a destination in virtual items of `members`; ext_front: the summands of
    a virtual item's inverse job = its members' parts + the tensor term).  Returns (summands per inverse job, highest c1 slot an item's parts name)."""
    items = []                                          # (destination, parts)
    for i in ids0:
        items.append((0, parts))
        items.append((1 + i, parts))
    for j in ids1:
        items.append((1 + j, 1))
    jobs = []
    for dst in dict.fromkeys(d for d, _ in items):      # destinations in the order of their first product
        mem = [p for d, p in items if d == dst]
        for k in range(0, len(mem), members):
            jobs.append(sum(mem[k:k + members]) + (1 if k == 0 else 0))
    n, nf2 = len(items), 2 * len(ids0)
    return jobs, n + nf2 * (parts - 1)


def test_inverse_job_summands_and_part_slots_for_every_party_count():
    """For every (n0, n1 <= 32, level) of PN15QP880 whose tail the engine would run through ntt16_f2_kernel (n0 <= F2_MAX_P, the folded tensor term: 2 n0 + n1 <=
    EXT_MAX_ITEMS, a plan on a 256- or 304-CU device): no inverse job adds more than VI_SUMS summands at its load (csrc/engine.hip ext_front throws
    otherwise: a legal call would fail) and the c1 slot index packed into 8 bits of f2_parts[i] stays at or below 255 -- with equal id sets (every
    party's slot holds its u product, its step-E product and the tensor term) and with disjoint ones."""
    shapes = 0
    for n0 in range(1, 17):
        for level in range(14):
            members = min(VI_MAX, 16 // 2, (NTT_MAX_SLOTS - (level + 1)) // 2)          # Context::ext_merge_members, two special primes
            for grid in (-256, -304):
                nwg, parts, _ = _probe(n0, level + 1, level + 3, [100] * (level + 3), grid)
                if nwg == 0:
                    continue
                assert parts <= _max_parts(n0)
                # Rotate / Conjugate of n0 >= 2 components (csrc/engine_ops.hip): n0 key products onto out_0 (c_0 is the ModDown's addend, no summand of
                # the inverse job), one CRS product per party slot, 2 n0 items and their parts behind them
                assert min(members, n0) * parts <= VI_SUMS and 2 * n0 + 2 * n0 * (parts - 1) <= 255
                for n1 in range(0, 33):
                    if 2 * n0 + n1 > EXT_MAX_ITEMS:
                        continue
                    layouts = [(list(range(n0)), list(range(n1)))]
                    if n0 + n1 <= 32:
                        layouts.append((list(range(n0)), list(range(n0, n0 + n1))))
                    for ids0, ids1 in layouts:
                        jobs, top = _tail_jobs(ids0, ids1, parts, members)
                        assert max(jobs) <= VI_SUMS, (n0, n1, level, parts, jobs)
                        assert top <= 255, (n0, n1, level, parts, top)
                        shapes += 1
    assert shapes > 1000


F2_RUN_COST, F2_PART_COST, F2_SLACK = 80, 8, 190       # csrc/ntt_kernels.h, in units of a pass = 100


def _cost(segs, parts, weights):
    """f2_build_schedule's cost of a cut: the longest workgroup (passes by weight + a quarter pass per run) + the parts the inverse NTT reads again"""
    nd = segs[:, :, 4].astype(np.int64)
    w = np.asarray(weights, dtype=np.int64)[segs[:, :, 1].astype(np.int64)]
    per_wg = (nd * w + (nd > 0) * F2_RUN_COST).sum(axis=1)
    return int(per_wg.max()) + F2_PART_COST * parts


@pytest.mark.parametrize("parties", [1, 2, 3, 4, 5, 8, 16])
def test_planned_grid_is_the_cheapest_cut_or_none(parties):
    # the engine's plan (round 6: the grid is chosen, not the CU count): the cheapest cut over all grids of at most 256 workgroups, taken when it stays
    # within F2_SLACK of an even deal over the chip (the fused launch loses to the pair of launches it replaces beyond) -- checked against a scan
    taken = 0
    for level in range(14):
        nb, nslots = level + 1, level + 1 + 2
        weights = [100] * nslots
        even = parties * nslots * 2 * nb * 100 // 256
        best = None
        for grid in range(1, 257):
            nwg, parts, segs = _probe(parties, nb, nslots, weights, grid)
            if nwg:
                c = _cost(segs, parts, weights)
                best = c if best is None or c < best else best
        nwg, parts, segs = _probe(parties, nb, nslots, weights, -256)
        if nwg == 0:
            assert best is None or best - even > F2_SLACK or nb < 2, (parties, level, best, even)      # (level 0, one digit: never fused)
            continue
        taken += 1
        assert _check(parties, nb, nslots, weights, -256) == parts
        assert _cost(segs, parts, weights) == best and best - even <= F2_SLACK, (parties, level, nwg, parts, best, even)
    assert taken >= 5


def test_planned_headline_is_the_whole_chip():
    nwg, parts, segs = _probe(4, 14, 16, [100] * 16, -256)
    assert nwg == 256 and parts == 2 and (segs[:, 0, 4] == 7).all()


def test_random_shapes():
    rng = np.random.default_rng(62)
    found = 0
    for _ in range(400):
        parties, nb = int(rng.integers(1, 17)), int(rng.integers(1, 40))
        nslots = int(rng.integers(1, 41))
        grid = int(rng.choice([32, 104, 256, 304]))
        weights = [int(x) for x in rng.integers(80, 160, nslots)]
        found += _check(parties, nb, nslots, weights, grid) > 0
    assert found > 50


def test_refusals():
    assert _probe(0, 14, 16, [100] * 16, 256)[0] == 0
    assert _probe(17, 14, 16, [100] * 16, 256)[0] == 0
    assert _probe(4, 14, 16, [0] * 16, 256)[0] == 0
    # four parties at level 6 on 256 workgroups: 504 passes, a group of 7 digits would be cut into four parts -- more than an inverse job with four
    # members adds at its load; the planned grid takes fewer workgroups
    assert _probe(4, 7, 9, [100] * 9, 256)[0] == 0
    # -- the plan does: fewer workgroups; not at level 6, where the cheapest cut leaves the longest workgroup too far above an even deal
    nwg, parts, _ = _probe(4, 8, 10, [100] * 10, -256)
    assert 0 < nwg < 256 and parts <= 3
    assert _probe(4, 7, 9, [100] * 9, -256)[0] == 0
    # three parties at the top level: 1344 passes, six for the longest workgroup where 5.25 would be even -- measured 3 % behind the unfused launches
    assert _probe(3, 14, 16, [100] * 16, -256)[0] == 0
