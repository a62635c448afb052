"""Shared pieces of the SemGCN posenet tests: the skeleton and its adjacency pattern, the seeded state and inputs, a stock-torch
container with the reference's parameter names whose forward is the einsum restatement of the layer, the records a run produces,
and the launch-shape constants of csrc/dhaug_graph.hip the multi-pass sizes are derived from.  No reference code; nothing here
imports the package under test."""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "posenet_gcn.npz")
GOLDEN_F32 = os.path.join(ROOT, "tests", "golden", "posenet_gcn_f32.npz")          # the reference class's own fp32 run

# ---- launch shape of the graph kernels (csrc/dhaug_graph.hip, include/dhaug.h) ----------------------------------------------------
MIX_BLOCK = 256              # work items (pose x channel vector) per workgroup
MIX_MAX_BLOCKS = 512         # DHAUG_GRAPH_MIX_MAX_BLOCKS: more items than MIX_BLOCK * MIX_MAX_BLOCKS and a thread takes a second pass
MIX_VEC = {torch.float32: 4, torch.bfloat16: 8}       # channels per item, by the source's type
ADJ_MAX_BLOCKS = 64          # DHAUG_GRAPH_ADJ_MAX_BLOCKS
MAX_PAIRS = 256              # DHAUG_GRAPH_MAX_PAIRS


def mix_items(poses, C, src_dtype, out_bf16, transpose=False):
    """work items of a mix launch: the host code's arithmetic restated"""
    width = 2 * C if transpose else C
    wpad = -(-width // 16) * 16 if out_bf16 else width
    cw = wpad - C if transpose else wpad
    return poses * -(-cw // MIX_VEC[src_dtype])


# ---- skeleton -----------------------------------------------------------------------------------------------------------------------
JOINTS = 16
PARENTS = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 8, 10, 11, 8, 13, 14]


def adj_mask():
    """(16, 16) bool: self loops and both directions of every joint-parent edge"""
    m = np.eye(JOINTS, dtype=bool)
    for i, p in enumerate(PARENTS):
        if p >= 0:
            m[i, p] = m[p, i] = True
    return m


def adj_matrix():
    """the row-normalised adjacency as the reference's adj_mx_from_edges(sparse=False) gives it: fp32 (16, 16)"""
    a = adj_mask().astype(np.float64)
    return torch.tensor(a / a.sum(1, keepdims=True), dtype=torch.float)


def pattern():
    """(rows, cols) of the mask in row-major order: the order of the elements of e"""
    r, c = np.nonzero(adj_mask())
    return r.tolist(), c.tolist()


# ---- records of the fixture ---------------------------------------------------------------------------------------------------------
SMALL = dict(hid=32, blocks=2, seed=21)          # record (a), B = 6 and 37, and record (c)
WIDE = dict(hid=128, blocks=4, seed=22)          # record (b), B = 96
ROWS_A, ROWS_B = (6, 37), 96
INIT = dict(hid=16, blocks=1, seed=5)            # init_<key>: the reference's own initialisation under torch.manual_seed(seed)


def shapes(hid, blocks, nnz=46):
    """state_dict key -> (shape, dtype) in the reference's order"""
    s = OrderedDict()

    def conv(name, cin, cout):
        s[name + ".W"] = ((2, cin, cout), torch.float32)
        s[name + ".e"] = ((1, nnz), torch.float32)
        s[name + ".bias"] = ((cout,), torch.float32)

    def layer(name, cin, cout):
        conv(name + ".gconv", cin, cout)
        for k in ("weight", "bias", "running_mean", "running_var"):
            s["%s.bn.%s" % (name, k)] = ((cout,), torch.float32)
        s[name + ".bn.num_batches_tracked"] = ((), torch.int64)

    layer("gconv_input.0", 2, hid)
    for i in range(blocks):
        layer("gconv_layers.%d.gconv1" % i, hid, hid)
        layer("gconv_layers.%d.gconv2" % i, hid, hid)
    conv("gconv_output", hid, 3)
    return s


def seeded_state(hid, blocks, seed):
    """W U(+-1/sqrt(in)), e N(1, 0.5^2) (no adjacency uniform), gamma U(0.5, 1.5), beta and the biases U(+-0.25), running
    statistics (0, 1)"""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    for k, (shp, dt) in shapes(hid, blocks).items():
        if k.endswith("num_batches_tracked"):
            v = np.zeros(shp, np.int64)
        elif k.endswith("running_mean"):
            v = np.zeros(shp, np.float32)
        elif k.endswith("running_var"):
            v = np.ones(shp, np.float32)
        elif k.endswith(".W"):
            v = ((rs.random_sample(shp) * 2 - 1) / np.sqrt(shp[1])).astype(np.float32)
        elif k.endswith(".e"):
            v = (1.0 + 0.5 * rs.standard_normal(shp)).astype(np.float32)
        elif k.endswith("bn.weight"):
            v = (rs.random_sample(shp) + 0.5).astype(np.float32)
        else:
            v = ((rs.random_sample(shp) * 2 - 1) * 0.25).astype(np.float32)
        out[k] = torch.from_numpy(v)
    return out


def make_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 16, 2, generator=g)
    t = 0.3 * torch.randn(B, 16, 3, generator=g)
    return x, t


def inputs_of(cfg, B):
    return make_inputs(B, cfg["seed"] + 100 + B)


# ---- the stock container: the reference's keys, the layer as an einsum ------------------------------------------------------------------
def mix_ref(H0, H1, A, bias=None):
    """z[b,i,:] = A[i,i] h0[b,i,:] + sum_{j != i} A[i,j] h1[b,j,:] + bias for (B, 16, C) operands"""
    d = torch.diagonal(A)
    z = torch.einsum("i,bic->bic", d, H0) + torch.einsum("ij,bjc->bic", A - torch.diag(d), H1)
    return z if bias is None else z + bias


def softmax_adjacency(e, dtype=None):
    r, c = pattern()
    a = torch.full((JOINTS, JOINTS), -9e15, dtype=e.dtype if dtype is None else dtype, device=e.device)
    a[r, c] = e.reshape(-1)
    return torch.softmax(a, dim=1)


class StockGraphConv(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.W = nn.Parameter(torch.zeros(2, cin, cout))
        nn.init.xavier_uniform_(self.W.data, gain=1.414)
        self.e = nn.Parameter(torch.ones(1, len(pattern()[0])))
        self.bias = nn.Parameter(torch.zeros(cout))
        self.bias.data.uniform_(-1.0 / cout ** 0.5, 1.0 / cout ** 0.5)

    def forward(self, x):
        return mix_ref(x @ self.W[0], x @ self.W[1], softmax_adjacency(self.e), self.bias)


class StockLayer(nn.Module):
    def __init__(self, cin, cout, p):
        super().__init__()
        self.gconv = StockGraphConv(cin, cout)
        self.bn = nn.BatchNorm1d(cout)
        self.p = p

    def forward(self, x):
        z = self.bn(self.gconv(x).transpose(1, 2)).transpose(1, 2)
        return nn.functional.dropout(torch.relu(z), self.p, self.training)


class StockBlock(nn.Module):
    def __init__(self, hid, p):
        super().__init__()
        self.gconv1 = StockLayer(hid, hid, p)
        self.gconv2 = StockLayer(hid, hid, p)

    def forward(self, x):
        return x + self.gconv2(self.gconv1(x))


class StockGCN(nn.Module):
    """the network from stock torch pieces under the reference's parameter names, created in the reference's order (the floor of
    the parity tests, the yardstick of the kernel tests and the other side of the checkpoint round trip)"""

    def __init__(self, hid, blocks, dropout=0.0):
        super().__init__()
        self.gconv_input = nn.Sequential(StockLayer(2, hid, dropout))
        self.gconv_layers = nn.Sequential(*[StockBlock(hid, dropout) for _ in range(blocks)])
        self.gconv_output = StockGraphConv(hid, 3)

    def forward(self, x):
        x = x.reshape(x.shape[0], 16, 2)
        return self.gconv_output(self.gconv_layers(self.gconv_input(x)))


def run_record(model, x, t):
    """what the fixture's records hold, in their order: out (training mode), loss, grad_<parameter>, buf_<buffer> after the forward,
    eval_out (evaluation-mode output after it); (name, tensor) pairs"""
    model.train()
    model.zero_grad()
    out = model(x)
    loss = nn.functional.mse_loss(out, t)
    loss.backward()
    rec = [("out", out.detach()), ("loss", loss.detach().reshape(1))]
    rec += [("grad_" + k, p.grad.detach().clone()) for k, p in model.named_parameters()]
    rec += [("buf_" + k, b.detach().clone()) for k, b in model.named_buffers()]
    model.eval()
    with torch.no_grad():
        rec.append(("eval_out", model(x).detach()))
    return rec


def network_ref(state, x, t, dtype=torch.float64, device="cpu"):
    """the plain-torch restatement on `state`: the records of run_record in `dtype` on `device`"""
    hid = state["gconv_output.W"].shape[1]
    blocks = sum(1 for k in state if k.endswith("gconv1.gconv.W"))
    m = StockGCN(hid, blocks)
    m.load_state_dict(state, strict=True)
    m = m.to(device=device, dtype=dtype)
    return run_record(m, x.to(device=device, dtype=dtype), t.to(device=device, dtype=dtype))


def load_golden(path=GOLDEN):
    z = np.load(path)
    return {k: z[k] for k in z.files}


# ---- comparing a run with a record ----------------------------------------------------------------------------------------------------
def scale_name(name, names):
    """the tensor whose largest element is the yardstick of `name`'s error: the tensor itself, except for the gradient of a
    SemGraphConv bias that a BatchNorm follows.  That gradient is identically zero (BatchNorm removes a per-channel constant): what
    a run returns is the rounding residue of the column sum of dz, whose terms have the size of the terms of the same layer's
    BatchNorm-bias gradient (the column sum of gz), so it is measured against that tensor."""
    if name.startswith("grad_") and name.endswith(".gconv.bias"):
        other = name[:-len(".gconv.bias")] + ".bn.bias"
        if other in names:
            return other
    return name


def errors_whole(rec, G, prefix):
    """max|t - ref| / max|yardstick| per floating tensor of rec against the whole-tensor records G[prefix + name]; integer tensors
    are compared exactly"""
    names = {n for n, _ in rec}
    out = OrderedDict()
    for n, v in rec:
        ref = torch.from_numpy(np.array(G[prefix + n]))
        if not ref.dtype.is_floating_point:
            assert int(v) == int(ref), n
            continue
        scale = torch.from_numpy(np.array(G[prefix + scale_name(n, names)])).double().abs().max().item()
        out[n] = (v.detach().double().cpu() - ref.double()).abs().max().item() / scale
    return out


def compact_ref(G, prefix, n):
    keys = [k for k in G if k.startswith("%s%s__" % (prefix, n))]
    return {k.rsplit("__", 1)[1]: torch.from_numpy(np.array(G[k])) for k in keys}


def errors_compact(rec, G, prefix):
    """the same against golden_util.compact records: sampled elements against the yardstick's largest sample, projections / (4 sqrt n)"""
    import golden_util as GU
    names = {n for n, _ in rec}
    out = OrderedDict()
    for i, (n, v) in enumerate(rec):
        if not v.dtype.is_floating_point:
            assert int(v) == int(G[prefix + n]), n
            continue
        ref, got = compact_ref(G, prefix, n), GU.compact(v, i)
        key = "full" if "full" in ref else "sample"
        sref = compact_ref(G, prefix, scale_name(n, names))
        scale = sref["full" if "full" in sref else "sample"].double().abs().max().item()
        e = (got[key].double() - ref[key].double()).abs().max().item() / scale
        if "proj" in ref:
            e = max(e, (got["proj"] - ref["proj"].double()).abs().max().item() / (4.0 * scale * v.numel() ** 0.5))
        out[n] = e
    return out
