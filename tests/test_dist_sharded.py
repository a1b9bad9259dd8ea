"""N>1 path: party-sharded MulAndRelin (mkhe_kklss_amd.dist) must reproduce the single-process result
bit for bit.

CPU (gloo, world_size 2, spawned processes): orchestration + collectives with the oracle doing the local
arithmetic.  GPU (-m gpu): the HIP backend through the split-phase C ABI (mkhe_mr_partial / mkhe_swk_fold /
mkhe_mr_finish / mkhe_ct_fold), ranks emulated one after the other on the single available GPU.
"""
import os
import socket
import sys

import numpy as np
import pytest

import harness as H
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_case(pset, names, seed, level=None):
    rng = np.random.default_rng(seed)
    ks = O.KeySwitcher(pset["logN"], pset["Q"], pset["P"], 2)
    level = len(pset["Q"]) - 1 if level is None else level
    k = len(names)
    op0, op1 = H.uniform_ct(rng, ks, k, level + 1), H.uniform_ct(rng, ks, k, level + 1)
    rlk = {n: tuple(H.uniform_swk(rng, ks) for _ in range(3)) for n in names}
    u = H.uniform_swk(rng, ks)
    ids = list(range(k))
    _, ref = ks.mul_and_relin(level, ids, op0, ids, op1, {i: rlk[n] for i, n in enumerate(names)}, u)
    return ks, level, op0, op1, rlk, u, ref


def test_assign_units():
    from mkhe_kklss_amd.dist import assign_units
    names = ["a", "b", "c", "d"]
    assert assign_units(names, 1) == [(names, names)]
    assert assign_units(names, 2) == [(["a", "b"], ["a", "b"]), (["c", "d"], ["c", "d"])]
    assert assign_units(names, 4) == [([n], [n]) for n in names]
    w8 = assign_units(names, 8)
    assert w8[0] == (["a"], []) and w8[1] == ([], ["a"]) and w8[7] == ([], ["d"])
    for world in (1, 2, 3, 4, 8):
        au = assign_units(names, world)
        assert sorted(sum((u[0] for u in au), [])) == names and sorted(sum((u[1] for u in au), [])) == names


def test_exact_sum_ok():
    """a sum formed inside a collective stays below 2^63 (the domain of mkhe_swk_fold / mkhe_ct_fold): 8 ranks of 60-bit residues, 16 of 59-bit ones"""
    from mkhe_kklss_amd.dist import exact_sum_ok
    q60, q59 = H.PN15QP880["Q"][0], H.PN15QP880["P"][0]
    assert q60.bit_length() == 60 and q59.bit_length() == 59
    assert exact_sum_ok(8, [q60]) and not exact_sum_ok(9, [q60])
    assert exact_sum_ok(16, [q59]) and not exact_sum_ok(17, [q59])
    assert exact_sum_ok(8, [q59, q60, 3]) and not exact_sum_ok(9, [3, q60, q59])          # the largest modulus decides
    assert exact_sum_ok(16, H.PN15QP880["Q"][1:] + H.PN15QP880["P"]) and not exact_sum_ok(16, H.PN15QP880["Q"] + H.PN15QP880["P"])


class _NineRanks:
    """stub of torch.distributed: a world of 9, and no collective may be reached"""

    class ReduceOp:
        SUM = "sum"

    def get_world_size(self, group=None):
        return 9

    def get_rank(self, group=None):
        return 0

    def __getattr__(self, name):
        raise AssertionError("collective %s reached" % name)


def test_all_reduce_refused_past_the_exact_sum_bound(oracle_lib):
    """small_ckks(10, 3) carries the 60-bit prime: nine ranks' sum of its residues can pass 2^63, so the all-reduce forms refuse before any work"""
    import torch
    from dist_oracle_backend import OracleRotateBackend, OracleShardBackend
    from mkhe_kklss_amd.dist import ShardedMulRelin, ShardedRotate
    names = ["u0", "u1"]
    pset = H.small_ckks(10, 3)
    ks, level, op0, op1, rlk, u, ref = make_case(pset, names, 3)
    b = OracleShardBackend(ks, names, 0, 9, op0, op1, rlk, u, level, torch)
    b.partial_xy = None                                                # refused before the rank's own arithmetic
    assert b.moduli() == pset["Q"] + pset["P"] and b.moduli(out=True) == pset["Q"]
    for mesh in (False, True):                                         # 15 limbs do not divide by 9, and the outputs are all-reduced either way
        with pytest.raises(ValueError) as e:
            ShardedMulRelin(b, _NineRanks(), mesh=mesh).run()
        assert "9 ranks" in str(e.value) and "%#x" % pset["Q"][0] in str(e.value)
    rb = OracleRotateBackend(ks, names, 0, 9, op0, {}, u, 5, level, torch)
    with pytest.raises(ValueError) as e:
        ShardedRotate(rb, _NineRanks()).run()
    assert "9 ranks" in str(e.value) and "%#x" % pset["Q"][0] in str(e.value)


def test_backend_without_moduli_is_held_to_the_largest_engine_modulus():
    """a backend that does not expose its moduli is checked against 2^60 - 1, the largest modulus an engine context admits: refused at 9 ranks,
    let through to its own arithmetic at 8"""
    from mkhe_kklss_amd.dist import MAX_ENGINE_MODULUS, ShardedRotate, exact_sum_ok

    class Reached(Exception):
        pass

    class Bare:
        def partial(self):
            raise Reached

    class EightRanks(_NineRanks):
        def get_world_size(self, group=None):
            return 8

    assert MAX_ENGINE_MODULUS == 2 ** 60 - 1 and exact_sum_ok(8, [MAX_ENGINE_MODULUS]) and not exact_sum_ok(9, [MAX_ENGINE_MODULUS])
    with pytest.raises(ValueError) as e:
        ShardedRotate(Bare(), _NineRanks()).run()
    assert "9 ranks" in str(e.value)
    with pytest.raises(Reached):
        ShardedRotate(Bare(), EightRanks()).run()


def _worker(rank, world, port, names, seed, out_path):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dist_oracle_backend import OracleShardBackend
    from mkhe_kklss_amd.dist import ShardedMulRelin
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ks, level, op0, op1, rlk, u, ref = make_case(H.small_ckks(10, 3), names, seed)
    b = OracleShardBackend(ks, names, rank, world, op0, op1, rlk, u, level, torch)
    full = ShardedMulRelin(b, dist).run()
    ok = bool((b.full == ref).all())
    dist.barrier()
    if rank == 0:
        np.save(out_path, np.array([ok]))
    else:
        assert ok
    dist.destroy_process_group()


def _mesh_worker(rank, world, port, names, seed, out_path, limbs, mesh):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dist_oracle_backend import OracleShardBackend
    from mkhe_kklss_amd.dist import ShardedMulRelin
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ks, level, op0, op1, rlk, u, ref = make_case(H.small_ckks(10, limbs), names, seed)
    b = OracleShardBackend(ks, names, rank, world, op0, op1, rlk, u, level, torch)
    sm = ShardedMulRelin(b, dist, mesh=mesh)
    sm.run()
    ok = bool((b.full == ref).all()) and sm.used_mesh == mesh
    dist.barrier()
    if rank == 0:
        np.save(out_path, np.array([ok]))
    else:
        assert ok
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("names", [["u0", "u1"], ["u0", "u1", "u2"]])
def test_sharded_mulrelin_gloo_world2(tmp_path, names):
    import torch.multiprocessing as mp
    out = str(tmp_path / "ok.npy")
    mp.spawn(_worker, args=(2, _free_port(), names, 42, out), nprocs=2, join=True)
    assert np.load(out)[0]


# Round 5: the rendezvous and every collective of the N > 1 paths at FIVE and EIGHT real processes, on the CPU (gloo, the oracle
# doing each rank's arithmetic) -- the GPU boxes of this pool admit six processes on their one card, so `--gpus 8` cannot be rehearsed there.
#   5 ranks, 3 parties: six half-party units on five ranks (the uneven split);  5 ranks, 5 parties: whole parties;
#   8 ranks, 4 parties: one half-party unit per rank -- the driver's `bench.py --gpus 8` at its default four parties.
@pytest.mark.parametrize("world,names,mesh", [(2, ["u0", "u1"], True), (4, ["u0", "u1", "u2"], True), (8, ["u0", "u1", "u2", "u3"], True), (4, ["u0", "u1"], False)])
def test_sharded_mulrelin_gloo_mesh_exchange(tmp_path, world, names, mesh):
    """x and y as reduce-scatter + all-gather over disjoint limb slices (round 6): 4 Q + 2 P limbs, 4 digits = 24 limbs of a switching
    key, which 2, 4 and 8 ranks divide -- every rank folds its own slice from the pieces of one all-to-all; and the all-reduce form on request."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "ok.npy")
    mp.spawn(_mesh_worker, args=(world, _free_port(), names, 23, out, 4, mesh), nprocs=world, join=True)
    assert np.load(out)[0]


@pytest.mark.parametrize("world,names", [(5, ["u0", "u1", "u2"]), (5, ["u0", "u1", "u2", "u3", "u4"]), (8, ["u0", "u1", "u2", "u3"])])
def test_sharded_mulrelin_gloo_world5_and_8(tmp_path, world, names):
    import torch.multiprocessing as mp
    from mkhe_kklss_amd.dist import assign_units
    units = assign_units(names, world)
    assert len(units) == world and sorted(sum((u[0] for u in units), [])) == names and sorted(sum((u[1] for u in units), [])) == names
    out = str(tmp_path / "ok.npy")
    mp.spawn(_worker, args=(world, _free_port(), names, 42 + world, out), nprocs=world, join=True)
    assert np.load(out)[0]


class _FakeDist:
    """emulates all_reduce(SUM) over backends that live in one process (single GPU available)"""

    def __init__(self, world):
        self.world, self.pending = world, []

    class ReduceOp:
        SUM = "sum"


@pytest.mark.gpu
@pytest.mark.parametrize("world,names", [(1, ["u0", "u1"]), (2, ["u0", "u1"]), (4, ["u0", "u1"]), (2, ["u0", "u1", "u2"]),
                                         (8, ["u0", "u1", "u2", "u3"])])        # the last one: `bench.py --gpus 8` at its default 4 parties (half-party units)
def test_sharded_mulrelin_device_emulated_ranks(world, names):
    import torch
    from mkhe_kklss_amd import mkckks
    from mkhe_kklss_amd.dist import HipShardBackend
    pset = H.small_ckks(11, 3)
    ks, level, op0, op1, rlk, u, ref = make_case(pset, names, 7)
    bs = []
    for r in range(world):          # one engine context per emulated rank, like one process per GPU
        params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
        params.AddCRS(-1, u)
        bs.append(HipShardBackend(params, names, r, world, op0, op1, rlk, level, torch, 0))
    # phase 1 on every "rank", then the all-reduce by hand, exactly as ShardedMulRelin.run orders it
    xs, ys = [], []
    for b in bs:
        x, y = b.partial_xy()
        b.before_collective()
        xs.append(x.clone()); ys.append(y.clone())
    sx, sy = sum(xs[1:], xs[0]), sum(ys[1:], ys[0])
    outs = []
    for b in bs:
        b.tx.copy_(sx); b.ty.copy_(sy)
        torch.cuda.synchronize()
        b.fold_xy()
        outs.append(b.finish().clone())
    tot = sum(outs[1:], outs[0])
    b = bs[0]
    b.tfull.copy_(tot)
    torch.cuda.synchronize()
    b.fold_out()
    assert (b.full.download() == ref).all()


@pytest.mark.gpu
@pytest.mark.parametrize("world,names", [(2, ["u0", "u1"]), (4, ["u0", "u1", "u2"]), (8, ["u0", "u1", "u2", "u3"])])        # 8: half-party units
def test_sharded_mulrelin_device_emulated_ranks_mesh(world, names):
    """the mesh exchange of ShardedMulRelin.run on the device: x and y as all-to-all of limb slices + mkhe_swk_fold_pieces on the rank's own slice
    (first_limb = rank * 24 / world > 0, `world` pieces) + all-gather, the collectives done by hand in run's order.  24 switching-key limbs."""
    import torch
    from mkhe_kklss_amd import mkckks
    from mkhe_kklss_amd.dist import HipShardBackend
    pset = H.small_ckks(11, 4)
    ks, level, op0, op1, rlk, u, ref = make_case(pset, names, 29)
    bs = []
    for r in range(world):
        params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
        params.AddCRS(-1, u)
        bs.append(HipShardBackend(params, names, r, world, op0, op1, rlk, level, torch, 0))
    xs, ys = [], []
    for b in bs:
        x, y = b.partial_xy()
        b.before_collective()
        xs.append(x.clone()); ys.append(y.clone())
    words = xs[0].numel()
    per = words // world
    assert words == 24 * ks.N and per * world == words and per % bs[0].limb_words() == 0

    def mesh_finish(which, parts):
        folded = []
        for r, b in enumerate(bs):
            recv = torch.cat([p[r * per:(r + 1) * per] for p in parts])       # all-to-all: piece p = rank p's slice r
            torch.cuda.synchronize()
            b.fold_pieces(which, recv, world, per, r * per, per)              # into the rank's own slice of x / y
            b.before_collective()
            t = b.tx if which == "x" else b.ty
            folded.append(t[r * per:(r + 1) * per].clone())
        whole = torch.cat(folded)                                             # all-gather
        for b in bs:
            (b.tx if which == "x" else b.ty).copy_(whole)
        torch.cuda.synchronize()

    mesh_finish("y", ys)
    for b in bs:
        b.finish_head()
    mesh_finish("x", xs)
    outs = [b.finish_tail().clone() for b in bs]
    tot = sum(outs[1:], outs[0])
    b = bs[0]
    b.tfull.copy_(tot)
    torch.cuda.synchronize()
    b.fold_out()
    assert (b.full.download() == ref).all()


@pytest.mark.gpu
def test_sharded_mulrelin_device_emulated_ranks_headline_ring():
    """PN15QP880 at full size, eight parties on two emulated ranks (four parties each): every rank's finish runs step F2 inside the Decompose NTT of its
    t_i (csrc/ntt16_f2_kernels.hip; round 6) behind a plain inner-product launch for its step-E items -- x comes from the other rank --, and the split
    finish (head with y, tail with x) gives the same bits as the oracle's single-device evaluation."""
    import torch
    from mkhe_kklss_amd import mkckks
    from mkhe_kklss_amd.dist import HipShardBackend
    pset = H.PN15QP880
    names = ["u%d" % i for i in range(8)]
    ks, level, op0, op1, rlk, u, ref = make_case(pset, names, 15)
    world = 2
    bs = []
    for r in range(world):
        params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
        params.AddCRS(-1, u)
        bs.append(HipShardBackend(params, names, r, world, op0, op1, rlk, level, torch, 0))
    xs, ys = [], []
    for b in bs:
        x, y = b.partial_xy()
        b.before_collective()
        xs.append(x.clone()); ys.append(y.clone())
    sx, sy = sum(xs[1:], xs[0]), sum(ys[1:], ys[0])
    outs = []
    for b in bs:
        b.ty.copy_(sy)
        torch.cuda.synchronize()
        b.fold_y()
        b.finish_head()
        b.tx.copy_(sx)
        torch.cuda.synchronize()
        b.fold_x()
        outs.append(b.finish_tail().clone())
    tot = sum(outs[1:], outs[0])
    b = bs[0]
    b.tfull.copy_(tot)
    torch.cuda.synchronize()
    b.fold_out()
    assert (b.full.download() == ref).all()


# ---------------------------------------------------------------- party-sharded Rotate
def make_rot_case(pset, names, seed, rot=3):
    rng = np.random.default_rng(seed)
    ks = O.KeySwitcher(pset["logN"], pset["Q"], pset["P"], 2)
    level = len(pset["Q"]) - 1
    ct = H.uniform_ct(rng, ks, len(names), level + 1)
    rk = {n: H.uniform_swk(rng, ks) for n in names}
    crs = H.uniform_swk(rng, ks)
    galEl = pow(5, rot, 2 * ks.N)
    ref = ks.rotate(level, galEl, list(range(len(names))), ct, [rk[n] for n in names], crs)
    return ks, level, ct, rk, crs, galEl, ref


def _rot_worker(rank, world, port, names, out_path):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dist_oracle_backend import OracleRotateBackend
    from mkhe_kklss_amd.dist import ShardedRotate
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ks, level, ct, rk, crs, galEl, ref = make_rot_case(H.small_ckks(10, 3), names, 9)
    b = OracleRotateBackend(ks, names, rank, world, ct, rk, crs, galEl, level, torch)
    out = ShardedRotate(b, dist).run()
    ok = bool((out == ref).all())
    dist.barrier()
    if rank == 0:
        np.save(out_path, np.array([ok]))
    else:
        assert ok
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 5, 8])          # 5 and 8 ranks, 3 parties: ranks that own no party take part in the all-reduce with zeros
def test_sharded_rotate_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    out = str(tmp_path / "ok.npy")
    mp.spawn(_rot_worker, args=(world, _free_port(), ["u0", "u1", "u2"], out), nprocs=world, join=True)
    assert np.load(out)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("hoisted", [False, True])
@pytest.mark.parametrize("world", [1, 2, 3, 8])          # 8 ranks, 3 parties: ranks without a party (the bench's rotate leg at --gpus 8)
def test_sharded_rotate_device_emulated_ranks(world, hoisted):
    import torch
    from mkhe_kklss_amd import mkrlwe
    from mkhe_kklss_amd.dist import HipRotateBackend
    pset = H.small_ckks(11, 3)
    names = ["u0", "u1", "u2"]
    ks, level, ct, rk, crs, galEl, ref = make_rot_case(pset, names, 11)
    bs = []
    for r in range(world):
        params = mkrlwe.Parameters(pset["logN"], pset["Q"], pset["P"], 2)
        bs.append(HipRotateBackend(params, names, r, world, ct, rk, params.AddCRS(3, crs), 3, level, torch, 0, hoisted=hoisted))
    parts = [b.partial().clone() for b in bs]
    tot = sum(parts[1:], parts[0])
    b = bs[0]
    b.tfull.copy_(tot)
    torch.cuda.synchronize()
    out = b.finish().download()
    assert (out == ref).all()


# ---------------------------------------------------------------- limb-sharded MulAndRelin
def test_assign_moduli():
    from mkhe_kklss_amd.dist import assign_moduli
    for world in (1, 2, 3, 4, 8):
        a = assign_moduli(14, 2, world)
        assert sorted(sum(a, [])) == list(range(16))
        assert max(len(x) for x in a) - min(len(x) for x in a) <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("world,names", [(1, ["u0", "u1"]), (2, ["u0", "u1"]), (3, ["u0", "u1", "u2"]), (5, ["u0"])])
def test_limb_sharded_mulrelin_device_emulated_ranks(world, names):
    """every emulated rank owns a subset of the moduli; the exchanges are summed by hand in the order
    LimbShardedMulRelin.run issues them; the result must equal the single-device evaluation bit for bit"""
    import torch
    from mkhe_kklss_amd import mkckks
    from mkhe_kklss_amd.dist import HipLimbBackend
    pset = H.small_ckks(11, 3)
    ks, level, op0, op1, rlk, u, ref = make_case(pset, names, 13)
    bs = []
    for r in range(world):
        params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
        params.AddCRS(-1, u)
        bs.append(HipLimbBackend(params, names, r, world, op0, op1, rlk, level, torch, 0))
    for ph in (1, 2, 3, 4):
        views = []
        for b in bs:
            v = b.phase(ph)
            b.before_collective()
            views.append(v)
        tot = sum((v.clone() for v in views[1:]), views[0].clone())
        for v in views:
            v.copy_(tot)
        torch.cuda.synchronize()
    for b in bs:
        assert (b.result().download() == ref).all()


def _limb_worker(rank, world, port, names, out_path):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dist_oracle_backend import OracleLimbBackend
    from mkhe_kklss_amd.dist import LimbShardedMulRelin
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ks, level, op0, op1, rlk, u, ref = make_case(H.small_ckks(10, 3), names, 17)
    b = OracleLimbBackend(ks, names, rank, world, op0, op1, rlk, u, level, torch)
    out = LimbShardedMulRelin(b, dist).run()
    ok = bool((out == ref).all())
    dist.barrier()
    if rank == 0:
        np.save(out_path, np.array([ok]))
    else:
        assert ok
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 5, 8])          # small_ckks(10, 3) has 3 + 2 moduli: with 8 ranks three of them own none
def test_limb_sharded_exchange_pattern_gloo(tmp_path, world):
    import torch.multiprocessing as mp
    out = str(tmp_path / "ok.npy")
    mp.spawn(_limb_worker, args=(world, _free_port(), ["u0", "u1"], out), nprocs=world, join=True)
    assert np.load(out)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("sync", ["stream", "host"])
def test_limb_sharded_with_rccl_world1(sync):
    """the real collective path on one GPU: a one-rank RCCL process group, the all-reduces forced, ordered on the
    engine's stream (torch.cuda.ExternalStream) or through the host; the result must still equal the oracle's"""
    import torch
    import torch.distributed as dist
    from mkhe_kklss_amd import mkckks
    from mkhe_kklss_amd.dist import HipLimbBackend, LimbShardedMulRelin
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        pset = H.small_ckks(12, 3)
        names = ["u0", "u1"]
        ks, level, op0, op1, rlk, u, ref = make_case(pset, names, 29)
        params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
        params.AddCRS(-1, u)
        b = HipLimbBackend(params, names, 0, 1, op0, op1, rlk, level, torch, 0, sync=sync)
        smr = LimbShardedMulRelin(b, dist, force_collectives=True)
        for _ in range(3):                     # back-to-back steps: nothing may overtake the collectives
            out = smr.run()
        params.sync()
        torch.cuda.synchronize()
        assert (out.download() == ref).all()
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("sync", ["stream", "host"])
def test_party_sharded_with_rccl_world1(sync):
    """the party-sharded legs through a REAL one-rank RCCL group with the collectives forced: MulRelin (asynchronous all-reduces of
    y and x, mkhe_mr_finish_head under the reduction of x, mkhe_mr_finish_tail), hoisted Rotate and the mkbfv MulRelinNew, ordered
    on the engine's stream (torch.cuda.ExternalStream) or through the host; back-to-back steps, results = the oracle's"""
    import torch
    import torch.distributed as dist
    import harness_bfv as HB
    from mkhe_kklss_amd import mkbfv, mkckks
    from mkhe_kklss_amd.dist import (HipBfvShardBackend, HipRotateBackend, HipShardBackend, ShardedBfvMulRelin, ShardedMulRelin,
                                     ShardedRotate)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        pset = H.small_ckks(12, 3)
        names = ["u0", "u1", "u2"]
        ks, level, op0, op1, rlk, u, ref = make_case(pset, names, 37)
        params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
        params.AddCRS(-1, u)
        b = HipShardBackend(params, names, 0, 1, op0, op1, rlk, level, torch, 0, sync=sync)
        smr = ShardedMulRelin(b, dist, force_collectives=True)
        for _ in range(3):                     # back-to-back steps: nothing may overtake the collectives
            smr.run()
        params.sync()
        torch.cuda.synchronize()
        assert (b.full.download() == ref).all()
        # hoisted Rotate
        ks, level, ct, rk, crs, galEl, rref = make_rot_case(pset, names, 39)
        rb = HipRotateBackend(params, names, 0, 1, ct, rk, params.AddCRS(3, crs), 3, level, torch, 0, hoisted=True, sync=sync)
        srot = ShardedRotate(rb, dist, force_collectives=True)
        for _ in range(3):
            out = srot.run()
        params.sync()
        torch.cuda.synchronize()
        assert (out.download() == rref).all()
        # mkbfv
        bset = HB.small_bfv(11, 3)
        bfv, bop0, bop1, brlk, bu, bref = make_bfv_case(bset, names, 45)
        bparams = mkbfv.Parameters(bset["logN"], bset["Q"], bset["QMul"], bset["P"], bset["T"])
        bparams.AddCRS(-1, bu)
        bb = HipBfvShardBackend(bparams, names, 0, 1, bop0, bop1, brlk, torch, 0, sync=sync)
        sb = ShardedBfvMulRelin(bb, dist, force_collectives=True)
        for _ in range(3):
            sb.run()
        bparams.sync()
        torch.cuda.synchronize()
        assert (bb.full.download() == bref).all()
    finally:
        dist.destroy_process_group()


def _two_rank_gpu_worker(rank, world, port, mode, out_path):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from mkhe_kklss_amd import mkckks
    from mkhe_kklss_amd.dist import HipLimbBackend, HipShardBackend, LimbShardedMulRelin, ShardedMulRelin
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)       # gloo moves CUDA tensors through the host
    pset = H.small_ckks(11, 3)
    names = ["u0", "u1", "u2"]
    ks, level, op0, op1, rlk, u, ref = make_case(pset, names, 31)
    params = mkckks.Parameters(pset["logN"], pset["Q"], pset["P"], pset["scale"])
    params.AddCRS(-1, u)
    if mode == "party":
        b = HipShardBackend(params, names, rank, world, op0, op1, rlk, level, torch, 0)
        ShardedMulRelin(b, dist).run()
        got = b.full.download()
    else:
        b = HipLimbBackend(params, names, rank, world, op0, op1, rlk, level, torch, 0, sync=mode)
        got = LimbShardedMulRelin(b, dist).run().download()
    ok = bool((got == ref).all())
    dist.barrier()
    if rank == 0:
        np.save(out_path, np.array([ok]))
    else:
        assert ok
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["host", "stream", "party"])
def test_two_real_ranks_on_one_gpu(tmp_path, mode):
    """two PROCESSES, each with its own engine context on GPU 0, exchanging through torch.distributed (gloo carries the
    device tensors through the host: the only single-GPU way to run world size 2 for real): limb sharding with both
    synchronisation modes, and party sharding"""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "ok.npy")
    mp.spawn(_two_rank_gpu_worker, args=(2, port, mode, out), nprocs=2, join=True)
    assert np.load(out)[0]


@pytest.mark.gpu
def test_bench_gpus_2_self_launch_on_one_gpu():
    """`python bench.py --gpus 2` with WORLD_SIZE unset must spawn its two ranks itself and print ONE JSON line with
    n_gpus == 2.  On a single-GPU box both ranks share GPU 0 and gloo carries the tensors through the host
    (MKHE_DIST_ONE_DEVICE / MKHE_DIST_BACKEND): the figures are meaningless, the path is the real one."""
    import json
    import subprocess
    env = dict(os.environ, MKHE_DIST_ONE_DEVICE="1", MKHE_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--params", "PN14QP439", "--parties", "2"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["rccl_ranks"] == 2 and out["scaling"] == "strong"
    assert out["value"] > 0 and out["steps"] == 2 and out["warmup"] == 1
    legs = out["config"]["legs"]
    assert {"party", "rotate_hoisted", "limb", "replicas"} <= set(legs) and all(v["ms_per_step"] > 0 for v in legs.values())
    # round 3: the line validates itself -- the sharded result equals rank 0's single-GPU evaluation of the same inputs and the CPU
    # oracle's (run on rank 0 after the timed legs), and the replica leg (weak scaling) stands beside the strong-scaling value
    assert out["config"]["matches_single_gpu"] is True
    assert out["cpu_baseline"] is not None and out["cpu_baseline"]["bit_exact_vs_gpu"] is True and out["cpu_baseline"]["value"] > 0
    assert legs["replicas"]["scaling"] == "weak" and legs["replicas"]["mulrelin_per_sec"] > 0


@pytest.mark.gpu
def test_bench_gpus_3_default_config_on_one_gpu():
    """the driver's N > 1 command line on the DEFAULT configuration (PN15QP880, 4 parties = 8 half-party units) with three real rank
    processes sharing GPU 0: an uneven split (3 + 3 + 2 units), the launcher starting its ranks before anything touches the GPU, one JSON
    line, the sharded result equal to the single-GPU one.  More ranks do not fit under pytest on this pool (at most 6 processes may hold one
    GPU: this process + the launcher's agent + the ranks); `profiles/r4_dist_5ranks.json` is the same command with five ranks, run on its own
    (VERDICT r3 item 5 asked for eight: the process guard of the GPU box kills the seventh)."""
    import json
    import subprocess
    env = dict(os.environ, MKHE_DIST_ONE_DEVICE="1", MKHE_DIST_BACKEND="gloo")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--steps", "2", "--warmup", "1", "--no-cpu"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 3 and out["config"]["rccl_ranks"] == 3 and out["config"]["matches_single_gpu"] is True
    assert out["config"]["params"] == "PN15QP880" and out["config"]["parties"] == 4 and out["value"] > 0


# ---------------------------------------------------------------- mkbfv, parties sharded (whole parties per rank)
def make_bfv_case(pset, names, seed):
    import harness_bfv as HB
    bfv = HB.make_bfv(pset)
    data = HB.uniform_bfv_inputs(pset, len(names), seed)
    ids = list(range(len(names)))
    _, ref = bfv.mul_relin_new(ids, data["op0"], ids, data["op1"], data["rlk"], data["u"])
    rlk = {n: data["rlk"][i] for i, n in enumerate(names)}
    return bfv, data["op0"], data["op1"], rlk, data["u"], ref


def _bfv_worker(rank, world, port, names, out_path):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import harness_bfv as HB
    from dist_oracle_backend import OracleBfvShardBackend
    from mkhe_kklss_amd.dist import ShardedBfvMulRelin
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    bfv, op0, op1, rlk, u, ref = make_bfv_case(HB.small_bfv(10, 3), names, 41)
    b = OracleBfvShardBackend(bfv, names, rank, world, op0, op1, rlk, u, torch)
    ShardedBfvMulRelin(b, dist).run()
    ok = bool((b.full == ref).all())
    dist.barrier()
    if rank == 0:
        np.save(out_path, np.array([ok]))
    else:
        assert ok
    dist.destroy_process_group()


@pytest.mark.parametrize("names", [["u0", "u1"], ["u0", "u1", "u2"]])
def test_sharded_bfv_mulrelin_gloo_world2(tmp_path, names):
    """mkbfv MulRelinNew with whole parties per rank: gloo, world size 2, the oracle's mkbfv blocks doing the local arithmetic"""
    import torch.multiprocessing as mp
    import socket as _s
    s = _s.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "ok.npy")
    mp.spawn(_bfv_worker, args=(2, port, names, out), nprocs=2, join=True)
    assert np.load(out)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("world,names", [(1, ["u0", "u1"]), (2, ["u0", "u1"]), (2, ["u0", "u1", "u2"]), (3, ["u0", "u1", "u2"])])
def test_sharded_bfv_mulrelin_device_emulated_ranks(world, names):
    """the HIP backend through mkhe_bfv_mr_partial / mkhe_swk_fold / mkhe_bfv_mr_finish / mkhe_ct_fold, ranks emulated one after
    the other on the one GPU, the collectives done by hand"""
    import torch
    import harness_bfv as HB
    from mkhe_kklss_amd import mkbfv
    from mkhe_kklss_amd.dist import HipBfvShardBackend
    pset = HB.small_bfv(11, 3)
    bfv, op0, op1, rlk, u, ref = make_bfv_case(pset, names, 43)
    bs = []
    for r in range(world):
        params = mkbfv.Parameters(pset["logN"], pset["Q"], pset["QMul"], pset["P"], pset["T"])
        params.AddCRS(-1, u)
        bs.append(HipBfvShardBackend(params, names, r, world, op0, op1, rlk, torch, 0))
    parts = []
    for b in bs:
        ts = b.partial_xy()
        b.before_collective()                  # engine stream -> host, as ShardedBfvMulRelin does before touching the sums
        parts.append([t.clone() for t in ts])
    torch.cuda.synchronize()
    sums = [sum((p[j] for p in parts[1:]), parts[0][j]) for j in range(4)]
    for b in bs:
        for j in range(4):
            b.txy[j].copy_(sums[j])
        torch.cuda.synchronize()
        b.fold_xy()
    fulls = [b.finish().clone() for b in bs]
    tot = sum(fulls[1:], fulls[0])
    bs[0].tfull.copy_(tot)
    torch.cuda.synchronize()
    bs[0].fold_out()
    assert (bs[0].full.download() == ref).all()
