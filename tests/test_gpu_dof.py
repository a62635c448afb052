"""DOF angle distributions on the GPU: dhaug_dof_histogram / dhaug_dof_pair_histogram against the numpy restatement of
tests/dof_util.py (integer words exact, extremes bit-exact, fp64 sums inside a derived bound), at the edges of the documented
partition; accumulation, reproducible bits, the skip rule, limit saturation, memory that must stay unwritten; the generator's
monitor hook, the dataset entry over the IK, and the reference's three drawing functions."""
import argparse

import numpy as np
import pytest
import torch

import dof_util as U
import ik_util as K

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A5A5A5A5A
PAIRS4 = [(8, 3), (0, 1), (5, 5), (2, 0)]


@pytest.fixture(scope="module")
def M():
    import dhaug_amd
    from dhaug_amd import ops
    from dhaug_amd.utils import dof_stats
    from dhaug_amd.models_Fk_GAN import Fk_generator, forward_kinematics_DH_model, special_operate
    return argparse.Namespace(ops=ops, lib=dhaug_amd._lib, S=dof_stats, gen=Fk_generator, fkm=forward_kinematics_DH_model,
                              special=special_operate)


def upload(a, extra=0):
    """(rows, D) numpy -> a device view of pitch D + extra whose pad columns are NaN"""
    rows, D = a.shape
    buf = torch.full((max(rows, 1), D + extra), float("nan"), dtype=torch.float32, device="cuda")
    buf[:rows, :D] = torch.from_numpy(a)
    return buf[:rows, :D]


def fields(M, record, D):
    off = M.lib.dof_record_offsets(D)
    w = record.cpu().numpy()
    f = w.view(np.float64)
    out = {k: w[off[k]:off[k] + D] for k in ("nan", "outside", "at_lo", "at_hi", "inf")}
    out.update({k: f[off[k]:off[k] + D] for k in ("min", "max", "sum", "sumsq")})
    out.update(rows=int(w[0]), skipped=int(w[1]), counts=w[off["counts"]:].reshape(D, U.BINS))
    return out


def check_record(M, record, D, ref):
    """every int64 word exact, min / max bit for bit, sum / sumsq inside the bound of dof_util.sum_bounds"""
    got = fields(M, record, D)
    assert (got["rows"], got["skipped"]) == (ref["rows"], ref["skipped"])
    for k in ("counts", "nan", "outside", "inf", "at_lo", "at_hi"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["counts"].sum(axis=1) + got["nan"], np.full(D, ref["rows"] - ref["skipped"]))
    for k in ("min", "max"):
        assert np.array_equal(got[k].view(np.int64), ref[k].astype(np.float64).view(np.int64)), (k, got[k], ref[k])
    bs, bq = U.sum_bounds(ref)
    es, eq = np.abs(got["sum"] - ref["sum"]), np.abs(got["sumsq"] - ref["sumsq"])
    print("FIGURE sum error / bound %.3g, sumsq error / bound %.3g" % ((es / np.maximum(bs, 1e-300)).max(),
                                                                         (eq / np.maximum(bq, 1e-300)).max()))
    assert (es <= bs).all() and (eq <= bq).all()


def edge_rows(M, D):
    rg = M.lib.DOF_BLOCK // D
    return {"one": 1, "step-1": rg - 1, "step": rg, "step+1": rg + 1,
            "multipass": M.lib.DOF_MAX_BLOCKS * M.lib.DOF_MIN_STEPS * rg + 1}


@pytest.mark.parametrize("extra", [0, 3])
@pytest.mark.parametrize("which", ["one", "step-1", "step", "step+1", "multipass"])
@pytest.mark.parametrize("D", [1, 33, 37, 64])
def test_counts_flags_extremes_and_sums(M, D, which, extra):
    rows = edge_rows(M, D)[which]
    if which == "multipass":
        rg, slabs, slab_rows = M.lib.dof_partition(rows, D)
        # one row more than a full grid of minimum-length slabs: the slabs grow by a step
        assert 1 < slabs <= M.lib.DOF_MAX_BLOCKS and slab_rows == (M.lib.DOF_MIN_STEPS + 1) * rg
    a = U.trial_angles(rows, D, seed=1000 * D + rows % 997)
    rec = M.ops.dof_histogram(upload(a, extra), M.ops.dof_record(D))
    check_record(M, rec, D, U.histogram(a))


def test_one_bin(M):
    n = 100000
    a = np.full((n, 37), 12.5, dtype=np.float32)
    d = M.S.DofDistribution(37, pairs=PAIRS4).add(upload(a))
    r = d.result()
    want = np.zeros((37, U.BINS), dtype=np.int64)
    want[:, 192] = n
    assert np.array_equal(r["counts"], want) and r["rows"] == n and r["skipped"] == 0
    assert (r["min"] == 12.5).all() and (r["max"] == 12.5).all()
    got = fields(M, d.record, 37)
    assert (got["sum"] == 12.5 * n).all() and (got["sumsq"] == 156.25 * n).all()          # both representable: exact
    assert (r["mean"] == 12.5).all() and (r["std"] == 0).all()
    tab = np.zeros((4, U.BINS, U.BINS), dtype=np.int64)
    tab[:, 192, 192] = n
    assert np.array_equal(r["pair_counts"], tab)
    assert np.array_equal(d.normalised()[:, 192], np.ones(37))


def test_accumulation_and_same_bits(M):
    a, b = U.trial_angles(1000, 37, seed=3), U.trial_angles(777, 37, seed=4)
    ab = np.concatenate([a, b])
    ta, tb, tab = upload(a), upload(b, 3), upload(ab)
    two = [M.S.DofDistribution(37, pairs=PAIRS4).add(ta).add(tb) for _ in range(2)]
    one = M.S.DofDistribution(37, pairs=PAIRS4).add(tab)
    # the same two calls on two fresh records: identical bytes in the whole record and every table
    assert torch.equal(two[0].record, two[1].record) and torch.equal(two[0].table, two[1].table)
    f2, f1 = fields(M, two[0].record, 37), fields(M, one.record, 37)
    for k in ("counts", "nan", "outside", "inf", "at_lo", "at_hi"):
        assert np.array_equal(f2[k], f1[k]), k
    for k in ("min", "max"):
        assert np.array_equal(f2[k].view(np.int64), f1[k].view(np.int64))
    assert (f2["rows"], f2["skipped"]) == (f1["rows"], f1["skipped"]) == (1777, 0)
    assert torch.equal(two[0].table, one.table)
    ref = U.histogram(ab)
    check_record(M, two[0].record, 37, ref)
    check_record(M, one.record, 37, ref)
    # zero() gives a fresh record back
    assert torch.equal(one.zero().record, M.ops.dof_record(37)) and int(one.table.abs().sum()) == 0


def test_skip_rule(M):
    rows, mr = 1501, 1e-4
    a = U.trial_angles(rows, 37, seed=5)
    g = np.random.default_rng(6)
    res = g.choice(np.array([0.0, 5e-5, mr, np.nextafter(np.float32(mr), np.float32(1)), 1e-3, np.nan, np.inf], dtype=np.float32),
                   size=rows)
    keep = U.kept_rows(rows, res, mr)
    assert keep[res == np.float32(mr)].all() and not keep[np.isnan(res)].any() and 0 < keep.sum() < rows
    d = M.S.DofDistribution(37, pairs=PAIRS4).add(upload(a), torch.from_numpy(res).cuda(), mr)
    ref = U.histogram(a, res, mr)
    assert ref["skipped"] == rows - keep.sum()
    check_record(M, d.record, 37, ref)
    check_record(M, M.ops.dof_histogram(upload(a[keep]), M.ops.dof_record(37)), 37, dict(U.histogram(a[keep])))
    assert np.array_equal(d.result()["pair_counts"], U.pair_tables(a, PAIRS4, res, mr))
    assert np.array_equal(d.result()["counts"], U.histogram(a[keep])["counts"])


@pytest.mark.parametrize("tol", [0.0, 0.5])
def test_saturation(M, tol):
    lo, hi = np.asarray(M.ops.IK_GENERATOR_LO, dtype=np.float32), np.asarray(M.ops.IK_GENERATOR_HI, dtype=np.float32)
    g = np.random.default_rng(7)
    rows = 900
    a = (lo + (hi - lo) * g.uniform(0, 1, size=(rows, 37))).astype(np.float32)
    lo_t, hi_t = (lo + np.float32(tol)).astype(np.float32), (hi - np.float32(tol)).astype(np.float32)
    kind = g.integers(0, 8, size=(rows, 37))
    for k, v in ((1, lo), (2, hi), (3, U.ulp_step(lo, True)), (4, U.ulp_step(hi, False)), (5, lo_t), (6, U.ulp_step(lo_t, True)),
                 (7, U.ulp_step(hi_t, False))):
        a = np.where(kind == k, np.broadcast_to(v, a.shape), a).astype(np.float32)
    dead = list(M.ops.IK_DEAD_SLOTS)
    assert (lo[dead] == 0).all() and (hi[dead] == 0).all()
    a[:, dead] = 0.0                                 # what the generator writes into the slots it pins at lo = hi = 0
    d = M.S.DofDistribution(37, limits=(lo.tolist(), hi.tolist()), tol=tol).add(upload(a))
    ref = U.histogram(a, lo=lo, hi=hi, tol=tol)
    check_record(M, d.record, 37, ref)
    r = d.result()
    assert (r["at_lo"][dead] == rows).all() and (r["at_hi"][dead] == rows).all()         # a pinned slot counts in both
    assert 0 < r["at_lo"][0] < rows and 0 < r["at_hi"][0] < rows


@pytest.mark.parametrize("which", ["one", "step-1", "step", "step+1", "multipass"])
def test_pairs(M, which):
    rows = edge_rows(M, 37)[which]
    a = U.trial_angles(rows, 37, seed=11 + rows % 13)
    d = M.S.DofDistribution(37, pairs=PAIRS4).add(upload(a, 3 if rows % 2 else 0))
    assert np.array_equal(d.result()["pair_counts"], U.pair_tables(a, PAIRS4))
    b = U.trial_angles(rows, 37, seed=12 + rows % 13, nans=False)
    r = M.S.DofDistribution(37, pairs=PAIRS4).add(upload(b)).result()
    for p, (i, j) in enumerate(PAIRS4):              # no NaN: the margins of a table are the two slots' histograms
        assert np.array_equal(r["pair_counts"][p].sum(axis=1), r["counts"][i])
        assert np.array_equal(r["pair_counts"][p].sum(axis=0), r["counts"][j])
    assert np.array_equal(np.diag(r["pair_counts"][2]), r["counts"][5]) and r["pair_counts"][2].sum() == rows


def test_unwritten_memory(M):
    D, rows, pad = 37, 3000, 64
    L = M.lib
    words, ws_words = L.dof_record_offsets(D)["words"], L.DOF_WORKSPACE_BYTES // 8
    tab_words = 2 * U.BINS * U.BINS
    big = torch.full((pad + words + pad + ws_words + pad + tab_words + pad,), POISON, dtype=torch.int64, device="cuda")
    rec = big[pad:pad + words]
    ws = big[pad + words + pad:pad + words + pad + ws_words]
    tab = big[pad + words + pad + ws_words + pad:][:tab_words]
    rec.copy_(M.ops.dof_record(D))
    tab.zero_()
    a = U.trial_angles(rows, D, seed=21)
    view = upload(a, 3)                              # NaN in the pad columns
    s = torch.cuda.current_stream().cuda_stream or None
    L.call("dhaug_dof_histogram", view.data_ptr(), rows, D, D + 3, None, 0.0, None, None, 0.0, rec.data_ptr(), ws.data_ptr(), s)
    M.ops.dof_pair_histogram(view, [(8, 3), (0, 1)], tab.view(2, U.BINS, U.BINS))
    outside = torch.ones_like(big, dtype=torch.bool)
    for t in (rec, ws, tab):
        o = (t.data_ptr() - big.data_ptr()) // 8
        outside[o:o + t.numel()] = False
    assert int(outside.sum()) == 4 * pad and bool((big[outside] == POISON).all())
    ref = U.histogram(a)
    check_record(M, rec.clone(), D, ref)             # the pad's NaN changed no `nan` count
    assert np.array_equal(tab.view(2, U.BINS, U.BINS).cpu().numpy(), U.pair_tables(a, [(8, 3), (0, 1)]))
    # the workspace: only the slabs' (4, 64) blocks may have been written
    slabs = L.dof_partition(rows, D)[1]
    assert bool((ws[slabs * 4 * L.DOF_MAX_SLOTS:] == POISON).all())
    # rows = 0 leaves a poisoned record untouched
    poisoned = torch.full((words,), POISON, dtype=torch.int64, device="cuda")
    empty = torch.empty((0, D), dtype=torch.float32, device="cuda")
    M.ops.dof_histogram(empty, poisoned)
    M.ops.dof_pair_histogram(empty, [(8, 3)], tab.view(2, U.BINS, U.BINS)[:1])
    assert bool((poisoned == POISON).all())
    assert np.array_equal(tab.view(2, U.BINS, U.BINS).cpu().numpy(), U.pair_tables(a, [(8, 3), (0, 1)]))


# ------------------------------------------------------------------------------------------------------------ generator hook
def _generator(M, B):
    args = argparse.Namespace(batch_size=B, random_seed=0, GAN_OUTPUT_DIM=35, GAN_whether_use_preAngle=True, Gen_DenseDim=32,
                              bone_len_scaler="different", whether_use_RT=True)
    torch.manual_seed(17)
    G = M.gen.Fk_Generator(None, args, "cuda").cuda()
    g = torch.Generator().manual_seed(18)
    G.boneLength = (torch.tensor(K.DEFAULT_LEN) * (0.8 + 0.4 * torch.rand(B, 15, generator=g))).cuda()
    return G, torch.randn(B, 128, generator=g).cuda()


def _monitor(M, every):
    return M.S.DofMonitor(M.S.DofDistribution(37, pairs=((8, 3),), limits=(M.ops.IK_GENERATOR_LO, M.ops.IK_GENERATOR_HI)), every)


def _offset():
    return torch.cuda.default_generators[torch.cuda.current_device()].get_offset()


def test_generator_hook_changes_nothing_and_counts_the_batch(M):
    B = 48
    G, z = _generator(M, B)

    def sampling():
        with torch.no_grad():
            return [G(z)]

    def autograd():
        return [G(z).detach()]

    def critics():
        return [t for t in G.sample_for_critics(z) if t is not None]

    for run in (sampling, autograd, critics):
        outs = []
        for mon in (None, _monitor(M, 1)):
            G.dof_monitor = mon
            torch.manual_seed(5)
            outs.append((run(), _offset()))
        (plain, off0), (watched, off1) = outs
        assert off0 == off1 and len(plain) == len(watched) and all(torch.equal(x, y) for x, y in zip(plain, watched)), run.__name__
        # what the monitor saw = the angles record_angles yields for the same input
        G.dof_monitor, G.record_angles = None, True
        G(z)
        G.record_angles = False
        ang = G.distribute_angle[0]
        assert tuple(ang.shape) == (B, 37)
        by_hand = _monitor(M, 1).distribution.add(ang)
        assert torch.equal(mon.distribution.record, by_hand.record) and torch.equal(mon.distribution.table, by_hand.table)
        assert mon.distribution.result()["rows"] == B


def test_generator_hook_schedule_and_capture(M):
    from dhaug_amd import autograd_ops as A
    B = 4
    G, z = _generator(M, B)
    mon = G.dof_monitor = _monitor(M, 500)
    with torch.no_grad():
        for n in range(1, 502):
            G(z)
            if n in (1, 2, 500, 501):
                assert G.train_num == n
                assert mon.distribution.result()["rows"] == (2 * B if n == 501 else B), n
        # inside a capture nothing is fed, and the replay works
        mon = G.dof_monitor = _monitor(M, 1)
        s = torch.full((B, 8), 0.05, device="cuda")
        want = G(z, bone_len_scaler=s).clone()
        assert mon.distribution.result()["rows"] == B
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        A.CAPTURE_ID = 1 << 40                       # (as graphs.GraphedCall: packed copies are re-made inside)
        try:
            with torch.cuda.graph(graph):
                out = G(z, bone_len_scaler=s)
        finally:
            A.CAPTURE_ID = 0
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)
        assert mon.distribution.result()["rows"] == B


@pytest.mark.parametrize("how", ["default", "args", "environment"])
def test_factories_attach_the_monitor_only_when_asked(M, monkeypatch, how):
    """my_get_poseFk_model and video_mode_my_get_poseFk_model: no monitor by default; with args.dof_monitor or DHAUG_DOF_MONITOR=1
    a DofMonitor (every 500, pair (8, 3), the generator's limits) on model_G, its accumulator in the dictionary, fed by a forward"""
    from test_gpu_models import make_args
    from dhaug_amd.models_Fk_GAN import model_fk_gan_train as T
    B, R = 8, 9
    monkeypatch.delenv("DHAUG_DOF_MONITOR", raising=False)
    if how == "environment":
        monkeypatch.setenv("DHAUG_DOF_MONITOR", "1")
    over = dict(dof_monitor=True) if how == "args" else {}
    g = torch.Generator().manual_seed(41)
    for frames in (1, R):
        if frames == 1:
            args = make_args(batch_size=B, **over)
            d = T.my_get_poseFk_model(args, None, M.fkm.Forward_Kinematics_DH_Model(args, ["S1"], None))
        else:
            args = make_args(batch_size=B, single_or_multi_train_mode="multi", architecture="3,3", **over)
            d = T.video_mode_my_get_poseFk_model(args, None, M.fkm.Forward_Kinematics_DH_Model(args, ["S1"], None), R)
        G = d["model_G"]
        if how == "default":
            assert G.dof_monitor is None and "dof_distribution" not in d
            continue
        mon, dist = G.dof_monitor, d["dof_distribution"]
        assert isinstance(mon, M.S.DofMonitor) and mon.every == 500 and mon.distribution is dist
        assert dist.D == 37 and dist.pairs == [(8, 3)] and dist.tol == 0.0 and dist.record.is_cuda
        want = torch.tensor([M.ops.IK_GENERATOR_LO, M.ops.IK_GENERATOR_HI], dtype=torch.float32)
        assert torch.equal(dist.limits.cpu(), want)
        G.boneLength = (torch.tensor(K.DEFAULT_LEN) * (0.8 + 0.4 * torch.rand(B * frames, 15, generator=g))).cuda()
        with torch.no_grad():
            out = G(torch.randn(B, 128, generator=g).cuda())
        assert tuple(out.shape) == ((B, 48) if frames == 1 else (B, R, 48))
        r = dist.result()
        assert r["rows"] == B * frames and r["skipped"] == 0 and int(r["pair_counts"].sum()) == B * frames
        assert (r["counts"].sum(axis=1) == B * frames).all() and (r["outside"] == 0).all()


# ------------------------------------------------------------------------------------------------------------ dataset, drop-ins
def test_dataset_plumbing(M):
    fk = M.fkm.Forward_Kinematics_DH_Model(argparse.Namespace(batch_size=2, random_seed=0), ["S1"], None)
    d = K.trial_fit_inputs(64)
    pose, init = d["pose"].cuda(), d["init"].cuda()
    got = fk.dof_distribution(pose, init=init)
    fit = fk.fit_pose(pose, init=init, schedule="coarse_to_fine")
    by_hand = M.S.DofDistribution(37, pairs=((0, 1),)).add(fit.angles37, fit.residual, 1e-4)
    assert torch.equal(got.record, by_hand.record) and torch.equal(got.table, by_hand.table)
    r = got.result()
    assert r["rows"] == 64 and r["rows"] - r["skipped"] == int((fit.residual <= 1e-4).sum())
    assert int(r["pair_counts"].sum()) == r["rows"] - r["skipped"]

    t = K.trial_track_inputs(5, K.ragged_lengths(5))
    lengths = [b - a for a, b in zip(t["offsets"], t["offsets"][1:])]
    seq = t["pose"].cuda()
    into = M.S.DofDistribution(37, pairs=((0, 1), (8, 3)))
    assert fk.dof_distribution(seq, lengths=lengths, into=into, iters=8) is into
    fit = fk.fit_sequences(seq, lengths, cold_start=True, iters=8)
    by_hand = M.S.DofDistribution(37, pairs=((0, 1), (8, 3))).add(fit.angles37, fit.residual, 1e-4)
    assert torch.equal(into.record, by_hand.record) and torch.equal(into.table, by_hand.table)
    r = into.result()
    assert r["rows"] == sum(lengths) and r["rows"] - r["skipped"] == int((fit.residual <= 1e-4).sum())
    # a list of sequences is the same call
    parts = [seq[a:b] for a, b in zip(t["offsets"], t["offsets"][1:])]
    again = fk.dof_distribution(parts, pairs=((0, 1), (8, 3)), iters=8)
    assert torch.equal(again.record, into.record) and torch.equal(again.table, into.table)


def test_drop_ins(M, tmp_path):
    args = argparse.Namespace(record_all_picture=False, checkpoint=str(tmp_path))
    g = np.random.default_rng(31)
    a = g.uniform(-179.0, 179.0, size=(300, 37)).astype(np.float32)
    a[::2] = np.trunc(a[::2])                        # integer-valued rows among fractional ones
    ref = U.histogram(a)["counts"].astype(np.float64)
    t = torch.from_numpy(a)
    for inp in (t, t.cuda(), t.reshape(300, 37, 1)):
        table = M.special.my_draw_DOF_angle_distribute(inp, "dof", args)
        assert table.shape == (37, U.BINS) and np.array_equal(table, ref / ref.max(axis=1, keepdims=True))
    p83 = M.special.my_draw_distribute_for_paper(t.cuda(), "gen", args)
    p01 = M.special.my_draw_original_dataset_distribute_for_paper(t, "data", args)
    assert p83.dtype == np.int64 and np.array_equal(p83, U.pair_tables(a, [(8, 3)])[0])
    assert np.array_equal(p01, U.pair_tables(a, [(0, 1)])[0])
    assert not list(tmp_path.iterdir())              # record_all_picture is off: nothing is drawn
