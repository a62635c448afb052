"""GPU: the 2D critic's fused bf16 inference program runs pose_layer_4 (no activation) and layer_last as ONE layer whose weights
are the product of the two fp32 matrices (dhaug_pack_wfrag_composed / a two-operand dhaug_wfrag_desc): accuracy against the
layer-by-layer bf16 path and an fp64 evaluation, the in-place re-pack, hipGraph capture, and what must NOT have changed (the
pair launch, the f16x3 program).

Accuracy margin: the composed program's distance from the fp64 logits may exceed the layer-by-layer bf16 path's own distance by
no more than that path's seed-to-seed spread (max / min of its distance over the eight seeds) -- the spread is measured by the
test itself, from the layered path alone."""
import argparse
import copy

import pytest
import torch

from test_gpu_models import make_args, maxabs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import dhaug_amd
    dhaug_amd._lib.lib()
    from dhaug_amd.models_Fk_GAN import Fk_discriminator, Fk_generator, forward_kinematics_DH_model
    return argparse.Namespace(gen=Fk_generator, dis=Fk_discriminator, fkm=forward_kinematics_DH_model)

SEEDS = range(8)


def _critic(M, D, seed):
    torch.manual_seed(100 + seed)
    return M.dis.Fk_2D_Discriminator(make_args(Dis_DenseDim_2D=D), 16).cuda()


def _x(B, seed):
    g = torch.Generator().manual_seed(200 + seed)
    return ((torch.rand(B, 32, generator=g) - 0.5) * 1.6).cuda()


def _fp64(D2, x):
    """the module's forward in fp64 on the CPU (Fk_2D_Discriminator.forward, R/models_Fk_GAN/Fk_discriminator.py:253-266)"""
    import torch.nn.functional as F
    m = copy.deepcopy(D2).cpu().double()
    x = x.detach().cpu().double()
    s = D2.slope
    d1 = F.leaky_relu(m.pose_layer_1(x), s)
    d2 = F.leaky_relu(m.pose_layer_2(d1), s)
    d3 = F.leaky_relu(m.pose_layer_3(d2) + d1, s)
    return m.layer_pred(F.leaky_relu(m.layer_last(m.pose_layer_4(d3)), s)).detach()


def _layered(D2, x):
    """the layer-by-layer bf16 path: forward() with a graph to build (the fused programs serve the no-graph passes only)"""
    assert torch.is_grad_enabled()
    return D2(x).detach()


@pytest.mark.parametrize("D,B", [(D, B) for D in (64, 256) for B in (1, 129, 300)])
def test_composed_program_accuracy(M, D, B):
    """max |logit - fp64 logit| per seed as measured on an MI355X (layered bf16 path | composed program; margin = layered max / min):
      D=64  B=1    7.89e-5 1.06e-4 5.80e-5 1.36e-4 5.64e-5 2.31e-4 2.27e-4 4.74e-4 | 4.52e-5 3.03e-4 1.15e-5 1.09e-4 1.30e-4 2.63e-4 3.59e-6 1.81e-4   8.40
      D=64  B=129  3.52e-4 5.12e-4 5.50e-4 3.79e-4 3.22e-4 5.27e-4 5.14e-4 5.66e-4 | 2.59e-4 6.16e-4 4.48e-4 5.10e-4 3.93e-4 4.54e-4 3.73e-4 3.52e-4   1.76
      D=64  B=300  3.76e-4 5.94e-4 5.53e-4 5.00e-4 3.69e-4 6.27e-4 5.14e-4 5.76e-4 | 3.19e-4 6.16e-4 5.86e-4 5.85e-4 3.93e-4 5.43e-4 3.73e-4 5.08e-4   1.70
      D=256 B=1    1.71e-4 1.50e-5 1.44e-4 2.43e-4 1.55e-4 1.50e-4 5.99e-6 2.00e-4 | 8.66e-5 3.36e-6 1.53e-4 7.23e-6 1.58e-4 1.59e-4 7.10e-5 1.42e-4   40.6
      D=256 B=129  3.15e-4 3.25e-4 3.91e-4 3.06e-4 2.94e-4 3.87e-4 3.34e-4 3.90e-4 | 3.15e-4 3.38e-4 3.26e-4 3.53e-4 2.90e-4 2.91e-4 3.37e-4 3.50e-4   1.33
      D=256 B=300  4.35e-4 4.72e-4 4.99e-4 4.18e-4 3.32e-4 4.06e-4 4.16e-4 3.90e-4 | 3.55e-4 3.38e-4 4.87e-4 4.18e-4 2.90e-4 3.15e-4 3.83e-4 3.50e-4   1.50"""
    from dhaug_amd import fused
    lay, com = [], []
    for seed in SEEDS:
        D2, x = _critic(M, D, seed), _x(B, seed)
        with torch.no_grad():
            f = fused.critic2d(D2, x)
        assert fused.D2_COMPOSED in D2._fused["bf16"].layers and "pose_layer_4" not in D2._fused["bf16"].layers
        l = _layered(D2, x)
        assert f.shape == l.shape == (B, 1)
        assert maxabs(f, l) <= 2e-2 * l.abs().max().item() + 1e-6
        ref = _fp64(D2, x)
        lay.append(maxabs(l, ref))
        com.append(maxabs(f, ref))
    spread = max(lay) / min(lay)
    print("D=%d B=%d  layered |err| per seed: %s" % (D, B, " ".join("%.3e" % v for v in lay)))
    print("D=%d B=%d composed |err| per seed: %s  (margin = layered max/min = %.3f)" % (D, B, " ".join("%.3e" % v for v in com), spread))
    for seed, (a, c) in enumerate(zip(lay, com)):
        assert c <= a * spread, (seed, c, a, spread)


@pytest.mark.parametrize("D", [64, 256])
def test_in_place_update_repacks_the_composite(M, D):
    """pose_layer_4.weight alone, then layer_last.bias alone, updated in place (same tensors, new _version: the batch re-pack):
    the logits of a freshly constructed FusedNet on a cloned module, bit for bit"""
    from dhaug_amd import fused, _lib
    D2, x = _critic(M, D, 0), _x(300, 0)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        before = fused.critic2d(D2, x).clone()
        for p in (D2.pose_layer_4.weight, D2.layer_last.bias):
            p.mul_(1.0 + 0.05 * torch.randn(p.shape, generator=g).to(p.device))
            calls = _lib.CALLS[0]
            got = fused.critic2d(D2, x).clone()
            assert _lib.CALLS[0] - calls == 2                        # ONE re-pack launch + the fused launch
            fresh = copy.deepcopy(D2)
            fresh.__dict__.pop("_fused", None)
            want = fused.critic2d(fresh, x)
            assert torch.equal(got, want)
            assert not torch.equal(got, before)
            before = got


def test_captured_update_and_forward_replays(M):
    """a hipGraph that holds an in-place weight update followed by fused.critic2d: every replay re-packs the composite from the
    weights it has just changed"""
    from dhaug_amd import fused, autograd_ops as A
    B = 256
    D2, x = _critic(M, 256, 1), _x(B, 1)
    eager = copy.deepcopy(D2)
    delta = (0.01 * torch.randn(256, 256, generator=torch.Generator().manual_seed(3))).cuda()
    with torch.no_grad():
        fused.critic2d(D2, x)                                        # the program and its blobs exist before the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        A.CAPTURE_ID = 1 << 40                                       # (as graphs.GraphedCall: packed copies are re-made inside)
        try:
            with torch.cuda.graph(graph):
                D2.pose_layer_4.weight.add_(delta)
                out = fused.critic2d(D2, x)
        finally:
            A.CAPTURE_ID = 0
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            eager.pose_layer_4.weight.add_(delta)
            assert torch.equal(eager.pose_layer_4.weight, D2.pose_layer_4.weight)
            assert torch.equal(out, fused.critic2d(eager, x))


def test_pair_launch_and_parity_program_unchanged(M):
    from dhaug_amd import fused, ops
    B = 300
    args = make_args(batch_size=B, Dis_DenseDim_3D=256, Dis_DenseDim_2D=256)
    torch.manual_seed(5)
    D3 = M.dis.Fk_3D_Discriminator("cuda", args).cuda()
    D2 = M.dis.Fk_2D_Discriminator(args, 16).cuda()
    import golden_util as GU
    x3 = GU.synth_pose16(B, seed=9)
    x3 = (x3 - x3[:, :1]).reshape(B, 48).cuda()
    x2 = _x(B, 2)
    _, kb = ops.kcs_forward(x3, True, f32=False, bf16_ld=32)
    with torch.no_grad():
        p3, p2 = M.dis.score_fake_pair(D3, D2, x3, kb, x2.reshape(B, 16, 2))
        assert torch.equal(p3, fused.critic3d(D3, x3, kcs=kb)) and torch.equal(p2, fused.critic2d(D2, x2))
        # f16x3 keeps every layer: LOAD + six GEMM units, packed from the six modules one by one
        fused.critics(D3, D2, x3, None, x2, "f16x3")
        net = D2._fused["f16x3"]
        assert list(net.layers) == ["pose_layer_1", "pose_layer_2", "pose_layer_3", "pose_layer_4", "layer_last", "layer_pred"]
        units, _ = fused.D2["program"](D2, net.layers, dict(x=x2), B)
        assert sum(u.kind == fused.GEMM for u in units) == 6
        # and so does the forward-with-save program (the backward reads d4)
        assert len(fused.critic2d_forward_save(D2, x2)["d"]) == 5
        assert "pose_layer_4" in D2._fused["bf16+save"].layers
