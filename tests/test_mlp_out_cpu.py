"""CPU checks of the fused bf16 kernel's vector copy-out (csrc/dhaug_out_copy.h, PLAN_VSTORE of csrc/dhaug_mlp.hip).

1. The element -> (row, column) mapping of the staging image is integer arithmetic, row = (e * magic(N)) >> 19 in 32 bits: walked
   here for EVERY element index below 128 * 64 and every N in 1..64 with numpy's uint32 (the kernel's v_mul_u32_u24 / shift), not
   only for the indices a tile uses (e < 128 N).
2. A model of one workgroup's copy (256 threads): every live float is written exactly once, nothing outside
   [0, rows_live * N) is written, 16-byte stores are 16-byte aligned, and no staging byte outside a live row's columns [0, N) is
   read.
3. The planner (dhaug_mlp_plan, host only): the bit is set for the contiguous outputs of an inference plan, at both places an
   output layer runs, and clear for a strided output, under DHAUG_MLP_NOVSTORE, for a base that is not 16-byte aligned and in a
   forward-with-save plan."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import mlp_lead_util as LG
import mlp_out_util as O
import mlp_unit_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    import dhaug_amd  # noqa: F401
    from dhaug_amd import _lib
    return _lib


def test_constants_match_the_sources():
    pkg = [d for d in os.listdir(ROOT) if d.endswith("_amd") and os.path.isdir(os.path.join(ROOT, d, "csrc"))][0]
    hdr = open(os.path.join(ROOT, pkg, "csrc", "dhaug_out_copy.h")).read()
    for name, want in (("OUTC_PITCH", O.OUTC_PITCH), ("OUTC_BM", O.OUTC_BM), ("OUTC_SHIFT", O.OUTC_SHIFT)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, hdr).group(1)) == want
    assert "(1u << OUTC_SHIFT) / (uint32_t)N + 1u" in hdr
    api = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    assert int(re.search(r"#define DHAUG_MLP_PLAN_VSTORE\s+\(1 << (\d+)\)", api).group(1)) == O.PLAN_VSTORE.bit_length() - 1


def test_row_mapping_is_exact_for_every_element_and_width():
    e = np.arange(O.OUTC_BM * 64, dtype=np.uint32)
    for N in range(1, 65):
        row = O.outc_row(e, N)
        assert np.array_equal(row.astype(np.int64), e.astype(np.int64) // N), N
        live = e[e < O.OUTC_BM * N]                                          # the indices a tile can hold
        want = (live.astype(np.int64) // N) * O.OUTC_PITCH + live.astype(np.int64) % N
        assert np.array_equal(O.outc_lds_byte(live, N).astype(np.int64), 4 * want), N


@pytest.mark.parametrize("threads", [256])
def test_copy_model_writes_each_live_float_once_and_reads_only_live_columns(threads):
    for N in list(range(1, 9)) + [31, 32, 33, 35, 63, 64]:
        for rows in (1, 2, 3, 127, 128):
            writes, reads = O.outc_model(N, rows, threads)
            hits = np.zeros(O.OUTC_BM * 64 + 8, dtype=np.int64)
            for first, n, vec in writes:
                assert not vec or first % 4 == 0
                hits[first:first + n] += 1
            total = rows * N
            assert (hits[:total] == 1).all() and not hits[total:].any(), (N, rows)
            assert sum(1 for w in writes if not w[2]) == total % 4            # only the ragged end leaves as dwords
            r = np.asarray(reads, dtype=np.int64) // 4
            assert ((r // O.OUTC_PITCH) < rows).all() and ((r % O.OUTC_PITCH) < N).all(), (N, rows)
            assert len(reads) <= 4 * threads * (O.OUTC_BM * 64 // 4 // threads)


def _out_words(lib, p, **kw):
    pl = LG.plans(lib, p, **kw)
    return [w for u, w in zip(p.units, pl) if u["kind"] == U.GEMM and (u["flags"] & U.F_OUT_F32)], pl


@pytest.mark.parametrize("N", O.NS)
def test_planner_sets_the_bit_for_contiguous_inference_outputs_only(lib, N):
    for build, stack in ((O.tail_program, True), (O.single_program, False)):
        with O.vstore(True):
            (w,), pl = _out_words(lib, build(N, 0))
            assert w & O.PLAN_VSTORE and w & O.PLAN_OUT
            assert bool(pl[1] & LG.PLAN_STACK) == stack                      # (the output layer really is a stack's tail / a single layer)
            for M in (1, 129, 65536):
                assert _out_words(lib, build(N, 0), M=M)[0][0] & O.PLAN_VSTORE
            (ws,), _ = _out_words(lib, build(N, 5))                          # strided rows
            assert ws & O.PLAN_OUT and not ws & O.PLAN_VSTORE
            assert ws == w & ~O.PLAN_VSTORE                                  # (nothing else of the word depends on it)
            if stack:                                                        # forward-with-save: the kernel of that launch has no such copy
                (wv,), _ = _out_words(lib, build(N, 0), save_at=1)
                assert not wv & O.PLAN_VSTORE
        with O.vstore(False):                                                # DHAUG_MLP_NOVSTORE
            (wo,), _ = _out_words(lib, build(N, 0))
            assert wo == w & ~O.PLAN_VSTORE


def test_planner_keeps_the_loop_for_an_unaligned_base(lib):
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    units = []
    for kind, kw in ((U.LOAD_F32, dict(dst=1, cols=64, ld=64, g=base)),
                     (U.GEMM, dict(src=1, dst=0, flags=U.F_OUT_F32, ksteps=4, n=3, w=base, bias=base, g=base + 4, ld=3))):
        m = lib.MlpUnit()
        m.kind, m.src, m.dst, m.res, m.src2 = kind, -1, -1, -1, -1
        for k, v in kw.items():
            setattr(m, k, v)
        units.append(m)
    out = (ctypes.c_int32 * 2)()
    with O.vstore(True):
        arr = (lib.MlpUnit * 2)(*units)
        assert lib.lib().dhaug_mlp_plan(arr, 2, 128, out) == 0 and not out[1] & O.PLAN_VSTORE and out[1] & O.PLAN_OUT
        units[1].g = base
        arr = (lib.MlpUnit * 2)(*units)
        assert lib.lib().dhaug_mlp_plan(arr, 2, 128, out) == 0 and out[1] & O.PLAN_VSTORE


def test_programs_are_exact_and_the_dot_scratch_starts_as_nan():
    """the exactness condition of mlp_unit_util (asserted inside ref()) holds for every program of the GPU test"""
    for N in O.NS:
        for lde in O.LD_EXTRA:
            for p in (O.tail_program(N, lde), O.single_program(N, lde)):
                assert p.ref()["bits"] < U.EXACT_BITS and p.tensors["y"]["ld"] == N + lde
    for N in O.DOT_NS:
        p = O.dot_program(N)
        assert p.ref()["bits"] < U.EXACT_BITS and np.isnan(p.tensors["nan"]["data"]).all()
        assert p.units[0]["dst"] == p.units[-1]["dst"] == 0                  # the NaN image lies where the partial sums go
    p = O.dot_program(100, pair=True)
    assert p.ref()["bits"] < U.EXACT_BITS


def test_the_pair_program_runs_as_a_pair(lib):
    pl = LG.plans(lib, O.dot_program(100, pair=True))
    assert pl[2] & (1 << 30)                                                 # PLAN_PAIR: the logits leave from gemm_pair's call site
