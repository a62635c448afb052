"""GPU tests of the copy-out of dhaug_mlp_forward's outputs (csrc/dhaug_mlp.hip): the 16-byte-group copy of an fp32 output whose rows
are contiguous (PLAN_VSTORE: store_output_linear, csrc/dhaug_out_copy.h) against the rolled loop, and the one-trip sum of a DOT_OUT
layer's partial sums (dot_output_once).

Exact-tier programs of tests/mlp_out_util.py against the fp64 reference of tests/mlp_unit_util.py, bit for bit (the exactness
condition, the route each program gets and the copy's index arithmetic are asserted without a GPU by tests/test_mlp_out_cpu.py).
M = 1, 3, 127, 128, 129, 300; N = 1, 3, 35, 64; ld == N and ld == N + 5 (which keeps the loop); both places an output layer runs:
behind a stack of two 256 -> 256 layers, and as a single K = 64 layer.  Every output lies in a NaN-filled tensor with two guard rows
behind row M - 1 and, where ld > N, guard columns: they must still be NaN.  Each launch runs with the new copy and with
DHAUG_MLP_NOVSTORE set; both equal the reference and each other, NaN filling included.

DOT_OUT layers of 20, 40, 70 and 100 features (one to four waves own a slice): the unit in front fills the scratch buffer with NaN,
so a partial sum of a wave that owns no slice -- never written -- is NaN, and a sum that reads it, or multiplies it by zero, shows."""
import sys
import os

import pytest
import torch

import mlp_out_util as O
import mlp_unit_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dhaug():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, ROOT)
    import dhaug_amd
    from dhaug_amd import _lib, ops  # noqa: F401
    return dhaug_amd


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("lde", O.LD_EXTRA)
@pytest.mark.parametrize("N", O.NS)
@pytest.mark.parametrize("site", ["tail", "single"])
def test_output_copy_matches_reference_and_rolled_loop(dhaug, site, N, lde):
    p = (O.tail_program if site == "tail" else O.single_program)(N, lde)
    dev = U.Device(p, dhaug)
    for M in O.MS:
        with O.vstore(True):
            on = dev.run(M)
        with O.vstore(False):
            off = dev.run(M)
        y = on["y"]
        assert y.shape == (M + 2, N + lde) and y.data_ptr() % 16 == 0        # (guard rows; guard columns where ld > N)
        U.compare(p, on, M)                                                  # the reference bit for bit, guards still NaN
        U.compare(p, off, M)
        assert torch.equal(_bits(on["y"]), _bits(off["y"])), (p.name, M)


@pytest.mark.parametrize("N,pair", [(n, False) for n in O.DOT_NS] + [(100, True)])
def test_logit_sum_is_bit_identical_and_reads_no_unowned_partial(dhaug, N, pair):
    p = O.dot_program(N, pair)
    dev = U.Device(p, dhaug)
    for M in O.MS:
        out = dev.run(M)
        assert out["logit"].shape == (M + 2, 3)
        U.compare(p, out, M)
