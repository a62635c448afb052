"""Which route does dhaug_mlp_forward give a program?  Asked through dhaug_mlp_plan (host only: the same validation and planning
pass, nothing launched), for the route "stack with its lead operand from global memory" (PLAN_LEADG, csrc/dhaug_mlp.hip): a bf16
LOAD of 32 / 48 columns and the stack whose lead it feeds run as one unit.  tests/test_gpu_mlp_lead_global.py runs the same
programs with the route on and off; this file is the proof that "on" really is the new route, and that every shape the kernel
must not take that way is refused."""
import os
import sys

import pytest

import mlp_lead_util as LG
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


def _places(lib, p, **kw):
    return LG.fused_places(p, LG.plans(lib, p, **kw))


@pytest.mark.parametrize("lde", [0, 8])
def test_shipped_critic_shapes_take_the_route_at_all_three_places(lib, lde):
    with LG.route(True):
        d3, d2 = LG.d3_shaped(lde), LG.d2_shaped(lde)
        assert [p for p in _places(lib, d3)] == [0, 9] and d3.units[9]["cols"] == 48 and d3.units[0]["cols"] == 32
        assert _places(lib, d2) == [0]
        for M in (1, 129, 65536):
            assert _places(lib, d3, M=M) == [0, 9]


@pytest.mark.parametrize("name", sorted(LG.FUSED))
def test_every_fused_test_program_takes_the_route(lib, name):
    build, nplaces = LG.FUSED[name]
    with LG.route(True):
        for lde in (0, 8):
            assert len(_places(lib, build(lde))) == nplaces
    assert len(_places(lib, LG.d3_cap(), M=U.M_CAP)) == 2


def test_switch_fp32_inputs_and_narrow_widths_keep_the_load(lib):
    for build, _ in LG.FUSED.values():
        with LG.route(False):                                                 # DHAUG_MLP_NOLEADG
            pl = LG.plans(lib, build())
            assert not any(w & LG.PLAN_LEADG for w in pl)
        with LG.route(True):
            assert pl != LG.plans(lib, build())                               # (the switch was what made the difference)
    with LG.route(True):
        # fp32 LOADs keep their unit; the 3D critic's KCS operand stays bf16 and is still taken
        assert _places(lib, LG.d2_shaped(dtype="f32")) == []
        assert _places(lib, LG.d3_shaped(dtype="f32")) == [0]
        assert _places(lib, LG.l48_r3(dtype="f32")) == []
        for D in (64, 128):                                                   # no run of 256 -> 256 layers: no stack, no lead
            for build in (LG.d3_shaped, LG.d2_shaped):
                pl = LG.plans(lib, build(D=D))
                assert not any(w & (LG.PLAN_LEADG | LG.PLAN_STACK) for w in pl)


def test_refused_shapes_keep_the_load(lib):
    with LG.route(True):
        # the first run layer takes its in-place residual from the buffer that holds the LOAD's image
        p = LG.refused_even()
        assert p.units[3]["res"] == p.units[1]["dst"] == 1 and _places(lib, p) == []
        # a STORE / a LOAD of parked rows anywhere in the program
        p = LG.refused_store()
        assert any(u["kind"] == U.STORE_BF16 for u in p.units) and _places(lib, p) == []
        pl = LG.plans(lib, p)
        assert all(w == 1 for u, w in zip(p.units, pl) if u["kind"] == U.LOAD_BF16)      # (they drain the stores first)
        # a narrow unit reads the LOAD's image too, in front of the lead or behind it
        for p in (LG.refused_reader(), LG.refused_reader_late()):
            assert sum(1 for u in p.units if u["kind"] == U.GEMM and u["src"] == 1 and u["K"] == 32) == 2
            assert _places(lib, p) == []
        # the scan of later readers proper: the lead has its run behind it, and the first run layer names the LOAD's buffer as src
        p = LG.refused_src()
        pl = LG.plans(lib, p)
        assert p.units[3]["src"] == p.units[1]["dst"] == 1 and p.units[3]["res"] == 0
        assert (pl[2] & LG.PLAN_STACK) and (pl[2] & 15) == 4 and ((pl[2] >> 4) & 63) == 2 and _places(lib, p) == []
        # 64 columns, and a lead of two chunks
        p = U.get("stack_l128_r6_even")
        assert _places(lib, p) == []


def test_forward_with_save_never_takes_the_route(lib):
    with LG.route(True):
        for build, nplaces in LG.FUSED.values():
            p = build()
            assert len(_places(lib, p)) == nplaces
            for i, u in enumerate(p.units):
                if u["kind"] == U.GEMM and not u["flags"]:                    # a save target on any layer that may have one
                    assert _places(lib, p, save_at=i) == [], (p.name, i)


def test_plan_validates_like_forward(lib):
    import ctypes
    L = lib.lib()
    out = (ctypes.c_int32 * 4)()
    arr = (lib.MlpUnit * 1)(lib.MlpUnit())
    assert L.dhaug_mlp_plan(arr, 0, 128, out) == -1 and L.dhaug_mlp_plan(None, 1, 128, out) == -1
    assert L.dhaug_mlp_plan(arr, 1, 128, None) == -1
    arr[0].kind = 7
    assert L.dhaug_mlp_plan(arr, 1, 128, out) == L.dhaug_mlp_forward(arr, 1, 128, None) == -1


@pytest.mark.parametrize("name", sorted(LG.FUSED) + sorted(LG.REFUSED) + ["d3_cap"])
def test_gpu_test_programs_are_exact_and_not_degenerate(name):
    """the condition of tests/mlp_unit_util.py that makes the GPU test's bit-for-bit comparison legitimate, for both row pitches"""
    build = LG.d3_cap if name == "d3_cap" else (LG.FUSED[name][0] if name in LG.FUSED else LG.REFUSED[name])
    for lde in (0, 8):
        p = LG.get(build, lde)
        r = p.ref()
        assert p.tier == 1 and 0 < r["bits"] < U.EXACT_BITS
        U.nondegenerate(p)
        for u in p.units:
            if u["kind"] == U.LOAD_BF16 and p.tensors[u["t"]]["data"] is not None and u["cols"] in (32, 48):
                assert p.tensors[u["t"]]["ld"] == u["cols"] + lde


def test_empty_batch_is_a_no_op_that_looks_at_no_unit(lib):
    """dhaug_mlp_forward at M = 0 returns 0 whatever the units hold (an empty tensor's pointer is null); nunits and the array
    itself are still checked, and dhaug_mlp_plan goes on validating at any M"""
    import ctypes
    L = lib.lib()
    arr = (lib.MlpUnit * 2)(lib.MlpUnit(), lib.MlpUnit())
    arr[0].kind, arr[0].dst, arr[0].cols, arr[0].ld = U.LOAD_BF16, 1, 32, 32            # g == NULL
    arr[1].kind, arr[1].src, arr[1].dst, arr[1].ksteps, arr[1].n = U.GEMM, 1, 0, 2, 256  # w == bias == NULL
    assert L.dhaug_mlp_forward(arr, 2, 0, None) == 0
    assert L.dhaug_mlp_forward(arr, 2, 128, None) != 0
    assert L.dhaug_mlp_forward(arr, 0, 0, None) == -1 and L.dhaug_mlp_forward(None, 2, 0, None) == -1
    assert L.dhaug_mlp_forward(arr, 2, -1, None) == -1
    out = (ctypes.c_int32 * 2)()
    assert L.dhaug_mlp_plan(arr, 2, 0, out) != 0
