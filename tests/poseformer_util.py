"""Shared pieces of the PoseFormer posenet tests: the configurations of the fixture's records, the seeded state and inputs, a
stock-torch container with the reference's parameter names (nn.Linear / nn.LayerNorm holders, F.layer_norm, F.gelu and softmax
attention written out), the records a run produces, record (c)'s loop data, and the launch constants of csrc/dhaug_attn.hip the
kernel tests' sizes are derived from.  No reference code; nothing here imports the package under test."""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import golden_util as GU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "posenet_poseformer.npz")
GOLDEN_F32 = os.path.join(ROOT, "tests", "golden", "posenet_poseformer_f32.npz")      # the reference class's own fp32 run

# ---- launch shape of the kernels (csrc/dhaug_attn.hip, include/dhaug.h) ---------------------------------------------------------------
LN_BLOCK = 256                # lanes of a LayerNorm workgroup
LN_MAX_COLS = 2048            # DHAUG_LAYERNORM_MAX_COLS
LN_MAX_BLOCKS = 256           # DHAUG_LAYERNORM_MAX_BLOCKS: row slices of the parameter-gradient partials
LN_PARTIAL_ROWS = 8           # DHAUG_LAYERNORM_PARTIAL_ROWS: row lanes per column of a slice at C <= 32 (half as many above)
ATTN_MAX_TOKENS = 81          # DHAUG_ATTN_MAX_TOKENS
ATTN_MAX_HEAD_DIM = 64        # DHAUG_ATTN_MAX_HEAD_DIM
ATTN_MAX_BLOCKS = 8192        # DHAUG_ATTN_MAX_BLOCKS
GELU_BLOCK = 256              # four-column items per GELU workgroup
GELU_MAX_BLOCKS = 2048        # DHAUG_GELU_MAX_BLOCKS: more items than GELU_BLOCK * GELU_MAX_BLOCKS and a thread takes a second pass

# ---- records of the fixture -----------------------------------------------------------------------------------------------------------
SMALL = dict(num_frame=3, num_joints=5, embed_dim_ratio=16, depth=2, num_heads=4, seed=31)      # record (a), B = 7 and 2
SMALL27 = dict(num_frame=27, num_joints=16, embed_dim_ratio=16, depth=1, num_heads=4, seed=32)  # record (a27), B = 3
REF9 = dict(num_frame=9, num_joints=16, embed_dim_ratio=32, depth=4, num_heads=8, seed=33)      # record (b), B = 6
LOOP = dict(SMALL, num_joints=16, seed=34)                                                      # record (c)
ROWS_A, ROWS_A27, ROWS_B = (7, 2), 3, 6
LAYOUTS = (9, 27)                                # keys_ / shapes_ / dtypes_ / param_count at the reference's configuration
INIT = dict(SMALL, num_joints=2, seed=5)         # init_<key>: torch.manual_seed(seed), construction, .apply(init_weights)
TRAIN = dict(n=160, batch=64, seed=35, lr=1e-3)  # record (c): 64, 64, 32 clips; flip and playback on: 12 steps
MLP_RATIO = 2.0
# what golden_util.compact keeps of a record's tensors: (a) every tensor up to 4 096 elements whole (all but the temporal blocks' four
# weight matrices), the others and records (a27), (b), (c) as samples + projections, so that each fixture stays below 1 MB
COMPACT = dict(a=dict(max_full=4096, samples=2048), a27=dict(max_full=2048, samples=1024), b=dict(max_full=2048, samples=1024),
               c=dict(max_full=2048, samples=1024))


def kwargs(cfg, drop_path_rate=0.0):
    """the constructor arguments of a configuration (the reference's and the module's alike)"""
    return dict(num_frame=cfg["num_frame"], num_joints=cfg["num_joints"], in_chans=2, embed_dim_ratio=cfg["embed_dim_ratio"],
                depth=cfg["depth"], num_heads=cfg["num_heads"], mlp_ratio=MLP_RATIO, qkv_bias=True, qk_scale=None,
                drop_path_rate=drop_path_rate)


def reference_cfg(frames):
    return dict(REF9, num_frame=frames)


def shapes(cfg):
    """state_dict key -> shape in the reference's order (all fp32)"""
    f, p, r, depth = cfg["num_frame"], cfg["num_joints"], cfg["embed_dim_ratio"], cfg["depth"]
    E = r * p
    s = OrderedDict()
    s["Spatial_pos_embed"] = (1, p, r)
    s["Temporal_pos_embed"] = (1, f, E)

    def lin(name, cin, cout):
        s[name + ".weight"], s[name + ".bias"] = (cout, cin), (cout,)

    def norm(name, dim):
        s[name + ".weight"], s[name + ".bias"] = (dim,), (dim,)

    lin("Spatial_patch_to_embedding", 2, r)
    for group, dim in (("Spatial_blocks", r), ("blocks", E)):
        for i in range(depth):
            b = "%s.%d." % (group, i)
            norm(b + "norm1", dim)
            lin(b + "attn.qkv", dim, 3 * dim)
            lin(b + "attn.proj", dim, dim)
            norm(b + "norm2", dim)
            lin(b + "mlp.fc1", dim, int(dim * MLP_RATIO))
            lin(b + "mlp.fc2", int(dim * MLP_RATIO), dim)
    norm("Spatial_norm", r)
    norm("Temporal_norm", E)
    s["weighted_mean.weight"], s["weighted_mean.bias"] = (1, f, 1), (1,)
    norm("head.0", E)
    lin("head.1", E, 3 * p)
    return s


def seeded_state(cfg, seed=None):
    """weights U(+-1/sqrt(fan_in)), LayerNorm gamma U(0.5, 1.5), every bias, LayerNorm beta and both position embeddings U(+-0.25)"""
    rs = np.random.RandomState(cfg["seed"] if seed is None else seed)
    out = OrderedDict()
    for k, shp in shapes(cfg).items():
        is_norm = "norm" in k or k.startswith("head.0")
        if k.endswith(".weight") and is_norm:
            v = rs.random_sample(shp) + 0.5
        elif k.endswith(".weight"):
            v = (rs.random_sample(shp) * 2 - 1) / np.sqrt(shp[1])
        else:
            v = (rs.random_sample(shp) * 2 - 1) * 0.25
        out[k] = torch.from_numpy(v.astype(np.float32))
    return out


def make_inputs(cfg, B, seed):
    """x (B, num_frame, num_joints, 2) and the target of the one output frame (B, 1, num_joints, 3)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cfg["num_frame"], cfg["num_joints"], 2, generator=g)
    t = 0.3 * torch.randn(B, 1, cfg["num_joints"], 3, generator=g)
    return x, t


def inputs_of(cfg, B):
    return make_inputs(cfg, B, cfg["seed"] + 100 + B)


def train_batches():
    """record (c)'s clips as multiframe_util.train_data lays them out: 3D targets (n, 1, 16, 3) with the root anywhere (the loop
    centres them), 2D clips of one receptive field (n, num_frame, 16, 2); batches of 64, 64, 32"""
    g = torch.Generator().manual_seed(TRAIN["seed"])
    n, B = TRAIN["n"], TRAIN["batch"]
    b3 = 0.3 * torch.randn(n, 1, 16, 3, generator=g) + torch.randn(n, 1, 1, 3, generator=g)
    b2 = 0.4 * torch.randn(n, LOOP["num_frame"], 16, 2, generator=g)
    return [(b3[i:i + B], b2[i:i + B]) for i in range(0, n, B)]


def key_third(bias):
    """the k third of a qkv bias (or of its gradient)"""
    C = bias.shape[0] // 3
    return bias[C:2 * C]


# ---- the stock container: the reference's keys, the transformer from torch functions ----------------------------------------------------
class StockBlock(nn.Module):
    def __init__(self, dim, heads, eps=1e-6):
        super().__init__()
        self.heads = heads
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = nn.Module()
        self.attn.qkv = nn.Linear(dim, 3 * dim)
        self.attn.proj = nn.Linear(dim, dim)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = nn.Module()
        self.mlp.fc1 = nn.Linear(dim, int(dim * MLP_RATIO))
        self.mlp.fc2 = nn.Linear(int(dim * MLP_RATIO), dim)

    def attention(self, x):
        S, N, C = x.shape
        hd = C // self.heads
        q, k, v = self.attn.qkv(x).view(S, N, 3, self.heads, hd).permute(2, 0, 3, 1, 4)
        w = torch.softmax(torch.einsum("shid,shjd->shij", q, k) * hd ** -0.5, dim=-1)
        return self.attn.proj(torch.einsum("shij,shjd->sihd", w, v).reshape(S, N, C))

    def forward(self, x, scale=(None, None)):
        """scale: per branch a (sequences,) tensor of mask / keep, or None"""
        y = self.attention(self.norm1(x))
        x = x + (y if scale[0] is None else y * scale[0].to(y.dtype).view(-1, 1, 1))
        y = self.mlp.fc2(F.gelu(self.mlp.fc1(self.norm2(x))))
        return x + (y if scale[1] is None else y * scale[1].to(y.dtype).view(-1, 1, 1))


class StockPoseFormer(nn.Module):
    """the network from stock torch pieces under the reference's parameter names, created in the reference's order (the floor of the
    parity tests, the yardstick of the loop test and the other side of the checkpoint round trip).  No drop path of its own: forward
    takes the branch scales (mask / keep per sequence) a test hands it."""

    def __init__(self, num_frame, num_joints, embed_dim_ratio, depth, num_heads, **unused):
        super().__init__()
        self.f, self.p, self.r = num_frame, num_joints, embed_dim_ratio
        E = embed_dim_ratio * num_joints
        self.Spatial_patch_to_embedding = nn.Linear(2, embed_dim_ratio)
        self.Spatial_pos_embed = nn.Parameter(torch.zeros(1, num_joints, embed_dim_ratio))
        self.Temporal_pos_embed = nn.Parameter(torch.zeros(1, num_frame, E))
        self.Spatial_blocks = nn.ModuleList([StockBlock(embed_dim_ratio, num_heads) for _ in range(depth)])
        self.blocks = nn.ModuleList([StockBlock(E, num_heads) for _ in range(depth)])
        self.Spatial_norm = nn.LayerNorm(embed_dim_ratio, eps=1e-6)
        self.Temporal_norm = nn.LayerNorm(E, eps=1e-6)
        self.weighted_mean = nn.Conv1d(num_frame, 1, 1)
        self.head = nn.Sequential(nn.LayerNorm(E), nn.Linear(E, 3 * num_joints))

    def forward(self, x, scales=None):
        f, p = self.f, self.p
        x = x.reshape(-1, f, p, 2)
        b = x.shape[0]
        none = [(None, None)] * (2 * len(self.blocks))
        scales = none if scales is None else scales
        h = self.Spatial_patch_to_embedding(x.reshape(b * f, p, 2)) + self.Spatial_pos_embed
        for blk, s in zip(self.Spatial_blocks, scales):
            h = blk(h, s)
        h = self.Spatial_norm(h).reshape(b, f, p * self.r) + self.Temporal_pos_embed
        for blk, s in zip(self.blocks, scales[len(self.Spatial_blocks):]):
            h = blk(h, s)
        h = self.weighted_mean(self.Temporal_norm(h))
        return self.head(h).view(b, 1, p, 3)


def stock_of(cfg, state=None):
    m = StockPoseFormer(**{k: v for k, v in cfg.items() if k != "seed"})
    m.load_state_dict(seeded_state(cfg) if state is None else state, strict=True)
    return m


def run_record(model, x, t):
    """what the fixture's records hold, in their order: out (training mode), loss, grad_<parameter>, eval_out (evaluation-mode
    output after it); (name, tensor) pairs"""
    model.train()
    model.zero_grad()
    out = model(x)
    loss = F.mse_loss(out, t)
    loss.backward()
    rec = [("out", out.detach()), ("loss", loss.detach().reshape(1))]
    rec += [("grad_" + k, p.grad.detach().clone()) for k, p in model.named_parameters()]
    model.eval()
    with torch.no_grad():
        rec.append(("eval_out", model(x).detach()))
    return rec


def network_ref(cfg, x, t, dtype=torch.float64, device="cpu", state=None):
    """the plain-torch restatement on the seeded state: the records of run_record in `dtype` on `device`"""
    m = stock_of(cfg, state).to(device=device, dtype=dtype)
    return run_record(m, x.to(device=device, dtype=dtype), t.to(device=device, dtype=dtype))


# ---- comparing a run with a record ----------------------------------------------------------------------------------------------------
def scale_name(name, names):
    """the tensor whose largest element is the yardstick of `name`'s error: the tensor itself, except for the gradient of
    weighted_mean.bias.  That bias adds one constant to every channel in front of head.0, a LayerNorm, which removes it: the
    gradient is identically zero, what a run returns is the rounding residue of a sum of the cotangent over clips and channels, and
    the same cotangent's sum against the normalised activations is the gradient of weighted_mean.weight, so it is measured against that."""
    if name == "grad_weighted_mean.bias" and "grad_weighted_mean.weight" in names:
        return "grad_weighted_mean.weight"
    return name


def compact_ref(G, prefix, n):
    """the parts golden_util.compact kept of tensor n of a record: full | sample, proj"""
    keys = [k for k in G if k.startswith("%s%s__" % (prefix, n)) and not k.endswith("__numel")]
    return {k.rsplit("__", 1)[1]: torch.from_numpy(np.array(G[k])) for k in keys}


def errors_compact(rec, G, prefix, tag):
    """max|t - ref| / max|yardstick| per tensor of rec against the golden_util.compact records G[prefix + name + '__' + part] made
    with COMPACT[tag]: whole tensors element by element, sampled ones at the samples and projections / (4 sqrt n)"""
    names = {n for n, _ in rec}
    out = OrderedDict()
    for i, (n, v) in enumerate(rec):
        ref, got = compact_ref(G, prefix, n), GU.compact(v, i, **COMPACT[tag])
        assert ref and set(ref) == set(got), (n, sorted(ref), sorted(got))
        key = "full" if "full" in ref else "sample"
        sref = compact_ref(G, prefix, scale_name(n, names))
        scale = sref["full" if "full" in sref else "sample"].double().abs().max().item()
        e = (got[key].double() - ref[key].double()).abs().max().item() / scale
        if "proj" in ref:
            e = max(e, (got["proj"] - ref["proj"].double()).abs().max().item() / (4.0 * scale * v.numel() ** 0.5))
        out[n] = e
    return out


def errors_between(G, prefix, G2, prefix2, names):
    """errors_compact's figures between two records of the same tensors (the reference's fp32 run against its fp64 run)"""
    out = OrderedDict()
    nameset = set(names)
    for n in names:
        a, b = compact_ref(G2, prefix2, n), compact_ref(G, prefix, n)
        key = "full" if "full" in b else "sample"
        sref = compact_ref(G, prefix, scale_name(n, nameset))
        scale = sref["full" if "full" in sref else "sample"].double().abs().max().item()
        e = (a[key].double() - b[key].double()).abs().max().item() / scale
        if "proj" in b:
            numel = int(G[prefix + n + "__numel"])
            e = max(e, (a["proj"].double() - b["proj"].double()).abs().max().item() / (4.0 * scale * numel ** 0.5))
        out[n] = e
    return out


def record_names(cfg):
    return ["out", "loss"] + ["grad_" + k for k in shapes(cfg)] + ["eval_out"]


def records(cfg):
    """tensors of a record: out, loss, one gradient per parameter, eval_out"""
    return 3 + len(shapes(cfg))


def load_golden(path=GOLDEN):
    z = np.load(path)
    return {k: z[k] for k in z.files}
