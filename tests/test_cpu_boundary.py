"""CPU-only checks of the boundary and the host logic (no compute calls: there is no GPU here)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_lib(verbose=False)
    ge.build_hostcheck(verbose=False)
    return ge


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(dhaug_[a-z0-9_]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol(built):
    import dhaug_amd
    lib = ctypes.CDLL(dhaug_amd._lib.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), "libdhaug.so does not export %s" % n
    lib.dhaug_version.restype = ctypes.c_int
    lib.dhaug_arch.restype = ctypes.c_char_p
    assert lib.dhaug_version() == 100 and lib.dhaug_arch() == b"gfx950"
    # every declared compute entry point has a ctypes signature in the binding (and nothing else is bound)
    bound = set(dhaug_amd._lib.SIGNATURES)
    assert bound == set(names) - {"dhaug_version", "dhaug_arch"}


def test_scratch_sizes_mirror_the_header(built):
    """the binding's scratch sizes are the header's (a short scratch is an out-of-bounds write on the device)"""
    from dhaug_amd import ops
    hdr = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    assert int(re.search(r"#define\s+DHAUG_CRITIC_SCALARS_SCRATCH\s+(\d+)", hdr).group(1)) == ops.CRITIC_SCALARS_SCRATCH
    from dhaug_amd import fused
    expr = re.search(r"#define\s+DHAUG_MLP_X3_WORKSPACE_BYTES\s+\(([0-9 *]+)\)", hdr).group(1)
    assert eval(expr) == fused.X3_WORKSPACE_BYTES


def test_fk_grid_caps_mirror_the_header(built):
    """the workgroup caps of the FK launches: header, source and the binding's mirror agree (tests/test_gpu_fk_tail.py computes its
    multi-pass sizes from the mirror: a changed cap cannot silently make those tests single-pass)"""
    import dhaug_amd
    lib = dhaug_amd._lib
    hdr = open(os.path.join(ROOT, "include", "dhaug.h")).read()
    src = open(os.path.join(os.path.dirname(lib.__file__), "csrc", "dhaug_fk.hip")).read()
    define = lambda n: int(re.search(r"#define\s+%s\s+(\d+)" % n, hdr).group(1))
    assert define("DHAUG_FK_MAX_BLOCKS") == lib.FK_MAX_BLOCKS == 10240
    assert define("DHAUG_GEN_TAIL4_MAX_BLOCKS") == lib.GEN_TAIL4_MAX_BLOCKS == 4096
    assert src.count("dhaug_stream_grid(ntiles, 1, DHAUG_FK_MAX_BLOCKS)") == 1                      # launch_tiles: the four one-wave entries
    assert src.count("dhaug_stream_grid(ntiles, 1, DHAUG_GEN_TAIL4_MAX_BLOCKS)") == 1               # the four-wave generator tail
    assert len(re.findall(r"dhaug_stream_grid\(", src)) == 2 and "constexpr int TILE = 64;" in src


def test_div1000_is_the_correctly_rounded_quotient(built):
    """div1000 (csrc/dhaug_fk_math.h), exhaustively over the integers of the jitter draw: k / 1000 as IEEE fp32 division gives it"""
    import numpy as np
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hostcheck", "_build", "libhostcheck.so"))
    k = np.arange(-200, 200, dtype=np.float32)
    out = np.full_like(k, 7.0)
    P = ctypes.POINTER(ctypes.c_float)
    lib.hostcheck_div1000(k.ctypes.data_as(P), out.ctypes.data_as(P), ctypes.c_long(len(k)))
    want = k / np.float32(1000)
    assert want.dtype == np.float32 and len(k) == 400
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))


def test_ablation_switches_need_an_ablation_build(tmp_path):
    """a development switch ("timing only, results wrong") cannot reach a product library: every such -D is a compile error
    without -DDHAUG_ABLATION_BUILD (csrc/dhaug_common.h), and build_lib ignores DHAUG_EXTRA_HIPFLAGS unless the environment
    names an ablation build"""
    import subprocess
    import __graft_entry__ as G
    assert G.ablation_flags({"DHAUG_EXTRA_HIPFLAGS": "-DX3_ABL_NOSPLIT"}) == []
    assert G.ablation_flags({}) == []
    assert G.ablation_flags({"DHAUG_ABLATION_BUILD": "1", "DHAUG_EXTRA_HIPFLAGS": "-DX3_ABL_NOSPLIT"}) == ["-DDHAUG_ABLATION_BUILD", "-DX3_ABL_NOSPLIT"]
    src = tmp_path / "probe.cpp"
    src.write_text('#include "dhaug_common.h"\nint main() { return 0; }\n')
    base = [G.HIPCC, "-x", "hip", "--cuda-host-only", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), "-I" + G.CSRC]
    ok = subprocess.run(base + [str(src)], capture_output=True, text=True)
    assert ok.returncode == 0, ok.stderr[-2000:]
    for d in ("X3_ABL_NOSPLIT", "ABL_NOWRITE", "SAVE_ABL_NULLSTORES", "T4_ABL_NOCOMPUTE", "X3_TIMING", "DHAUG_MLP_TIMING"):
        bad = subprocess.run(base + ["-D" + d, str(src)], capture_output=True, text=True)
        assert bad.returncode != 0 and "DHAUG_ABLATION_BUILD" in bad.stderr, d
        good = subprocess.run(base + ["-D" + d, "-DDHAUG_ABLATION_BUILD", str(src)], capture_output=True, text=True)
        assert good.returncode == 0, (d, good.stderr[-2000:])
    # the shipped sources name no switch the guard does not know: every *_ABL_* / X3_* / timing macro tested by an #if / #ifdef
    guard = open(os.path.join(G.CSRC, "dhaug_common.h")).read()
    known = set(re.findall(r"defined\((\w+)\)", guard))
    internal = {"X3_NW", "X3_MT", "X3_BM", "X3_B16", "X3_THREADS", "X3_LDS_BYTES", "X3_MAX_UNITS", "X3_CASE", "X3_CASE_ADD",
                "X3_CASE_STASH", "X3_STAMP", "X3_WORKSPACE_BYTES"}                     # defined by the sources themselves, unconditionally
    for path in sorted(p for p in os.listdir(G.CSRC) if p.endswith((".hip", ".h"))):
        text = open(os.path.join(G.CSRC, path)).read()
        for mac in set(re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)[^\n]*?\b((?:\w*_ABL_\w+|ABL_\w+|X3_\w+|\w*TIMING\w*|\w+_OVERRIDE|W_NO_\w+))\b", text, re.M)):
            assert mac in known or mac in internal, (path, mac)
    # ... and the guard knows no switch that the sources have lost: every name in it occurs in another file of csrc/
    others = "".join(open(os.path.join(G.CSRC, p)).read() for p in sorted(os.listdir(G.CSRC)) if p.endswith((".hip", ".h")) and p != "dhaug_common.h")
    for mac in sorted(known):
        assert re.search(r"\b%s\b" % mac, others), mac


def test_argument_errors_are_returned_not_thrown(built):
    """host-side validation happens before any launch, so it can be exercised without a GPU"""
    import dhaug_amd
    L = dhaug_amd._lib.lib()
    assert L.dhaug_fk_forward(None, None, None, None, 4, 16, None) == -1             # null pointers
    assert L.dhaug_fk_forward(None, None, None, None, 0, 16, None) == 0              # empty batch is a no-op
    assert L.dhaug_fk_forward(None, None, None, None, 4, 17, None) == -1             # bad out_joints
    buf = (ctypes.c_float * 64)()
    mis = ctypes.c_void_p(ctypes.addressof(buf) + 4)
    assert L.dhaug_fk_forward(mis, mis, mis, mis, 1, 16, None) == -2                 # misaligned
    assert L.dhaug_gemm_bf16(mis, 8, mis, 8, None, None, 0, None, 0, None, 0, 0, None, 0, 4, 4, 24, 0, 0.0, None) in (-1, -3)
    # every pointer of the FK entries that moves as 16-byte vectors, one misaligned call each; the others are aligned HOST addresses,
    # so a call that got as far as a launch would return a HIP error, not -2
    fkb = (ctypes.c_float * 1024)()
    al = ctypes.c_void_p((ctypes.addressof(fkb) + 15) & ~15)
    for off in (4, 8):
        m = ctypes.c_void_p(al.value + off)
        assert L.dhaug_fk_backward(al, al, m, al, al, al, 1, None) == -2                                  # grad_out16
        assert L.dhaug_gen_tail_backward(al, al, al, m, al, 1, 1, None) == -2                             # grad_fake16
        assert L.dhaug_gen_tail_backward(al, al, None, m, al, 1, 0, None) == -2
        assert L.dhaug_gen_tail_forward(al, al, al, m, al, 1, 1, None) == -2                              # fake16
        assert L.dhaug_gen_tail_forward(al, al, None, m, None, 1, 0, None) == -2
        crit = lambda fake=al, cen=al, kcs=al, proj=al, so=None, draw=0: L.dhaug_gen_tail_forward_critics(
            al, al, None, fake, cen, kcs, al, al, al, proj, draw, 1, 2, so, 1, 1, 0, None)
        assert crit(fake=m) == -2 and crit(cen=m) == -2 and crit(kcs=m) == -2 and crit(proj=m) == -2
        assert crit(so=m, draw=1) == -2 and crit(so=m) == -2                                              # scaler_out, drawn or not
        assert crit(fake=m, cen=None, kcs=None, proj=None) == -2 and crit(cen=m, kcs=None, proj=None) == -2
    m2 = ctypes.c_void_p(al.value + 2)
    assert L.dhaug_gen_tail_forward_critics(al, al, None, al, None, m2, None, None, None, None, 0, 0, 0, None, 1, 1, 1, None) == -2
    assert L.dhaug_gen_tail_forward_critics(al, al, al, al, al, al, None, None, None, None, 1, 0, 0, None, 1, 1, 0, None) == -1   # draw and scaler
    assert L.dhaug_gen_tail_forward_critics(al, al, None, al, al, al, None, None, None, al, 0, 0, 0, None, 1, 1, 0, None) == -1   # proj2d, no camera
    # the round-6 entries: argument checks of the planes products and of the contraction's planes fields (no launch is reached)
    big = (ctypes.c_float * 4096)()
    a16 = ctypes.c_void_p((ctypes.addressof(big) + 15) & ~15)
    assert L.dhaug_gemm_bf16x6_planes(a16, 768, a16, 1536, None, None, 0, None, 0, 0, 0.0, a16, 256, None, 0, 4, 256, 256, 3, 0, 0.0, None) == -1      # x_order 3
    assert L.dhaug_gemm_bf16x6_planes(a16, 768, a16, 1536, None, None, 0, None, 0, 0, 0.0, a16, 256, None, 0, 4, 256, 192, 0, 0, 0.0, None) == -3      # piece width not 64 * 2^j
    assert L.dhaug_gemm_bf16x6_planes(a16, 512, a16, 1536, None, None, 0, None, 0, 0, 0.0, a16, 256, None, 0, 4, 256, 256, 0, 0, 0.0, None) == -2      # lda < 3 kp
    assert L.dhaug_gemm_bf16x6_planes(a16, 768, a16, 1536, None, None, 0, None, 0, 0, 0.0, a16, 256, None, 0, 0, 256, 256, 0, 0, 0.0, None) == 0       # empty batch
    assert L.dhaug_gemm_f16x3_planes(a16, 512, 1, a16, 768, None, None, 0, a16, 256, None, 0, 0, 4, 256, 200, 0, 0.0, None) == -3                        # planes need 64 * 2^j
    assert L.dhaug_gemm_f16x3_planes(a16, 512, 1, a16, 768, None, None, 0, a16, 256, a16, 256, 256, 4, 256, 256, 0, 0.0, None) == -2                     # ld_planes < 2 planes_kp
    assert L.dhaug_gemm_f16x3_planes(a16, 512, 1, a16, 768, None, None, 0, a16, 256, a16, 512, 248, 4, 256, 256, 0, 0.0, None) == -2                     # planes_kp < N
    assert L.dhaug_gemm_f16x3_planes(a16, 512, 1, a16, 768, None, None, 0, a16, 256, a16, 528, 260, 4, 256, 256, 0, 0.0, None) == -2                     # planes_kp % 8 != 0
    assert L.dhaug_gemm_f16x3_planes(a16, 512, 1, a16, 768, None, None, 0, a16, 256, a16, 516, 256, 4, 256, 256, 0, 0.0, None) == -2                     # ld_planes % 8 != 0
    assert L.dhaug_gemm_f16x3_planes(a16, 192, 1, a16, 288, None, None, 0, a16, 256, a16, 512, 256, 4, 256, 96, 0, 0.0, None) == -3                      # a_planes with kp = 96: not 64 * 2^j
    # a piece width that is no power of two passes the checks (an empty batch: the widths are judged, nothing is launched) ...
    assert L.dhaug_gemm_f16x3_planes(a16, 512, 1, a16, 768, None, None, 0, a16, 520, a16, 1552, 776, 0, 520, 256, 0, 0.0, None) == 0
    assert L.dhaug_gemm_f16x3_planes(a16, 512, 1, a16, 768, None, None, 0, a16, 520, a16, 1552, 512, 0, 520, 256, 0, 0.0, None) == -2                    # ... where planes_kp < N does not
    assert L.dhaug_split_bf16(a16, 64, a16, 4, 64, 64, 2, 3, None) == -1                                                                                # mode 2 is a six-term layout
    lay = (dhaug_amd._lib.TnLayer * 1)()
    lay[0].A, lay[0].lda, lay[0].B, lay[0].ldb = a16.value, 64, a16.value, 64
    lay[0].C, lay[0].ldc, lay[0].M, lay[0].N1, lay[0].N2 = a16.value, 64, 64, 64, 64
    lay[0].planes_a = 3
    assert L.dhaug_gemm_tn_group_bf16(lay, 1, a16, None) == -1                                                                                          # planes_a out of range
    lay[0].planes_a, lay[0].M = 2, 64                                                                                                                    # planes: M must be 6 x rows
    assert L.dhaug_gemm_tn_group_bf16(lay, 1, a16, None) == -1
    with pytest.raises(RuntimeError):
        dhaug_amd._lib.check(-2, "x")


def test_pose_and_elem_argument_errors(built):
    """the pose / camera / WGAN-GP / video entry points (csrc/dhaug_pose.hip, csrc/dhaug_elem.hip): a bad argument comes back as the
    documented code before any launch -- every pointer here is a valid HOST address, so a call that got as far as a launch would
    return a HIP error, not -1 / -2 -- and an empty batch is a no-op that looks at no pointer"""
    import dhaug_amd
    L = dhaug_amd._lib.lib()
    buf = (ctypes.c_float * 4096)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b = ctypes.c_void_p(base), ctypes.c_void_p(base + 4096)
    EINVAL, EALIGN = -1, -2
    # frame_diff: R >= 2, w >= 1, in_w >= w, rows >= 0
    assert L.dhaug_frame_diff(a, b, 4, 1, 48, 48, 0, None) == EINVAL
    assert L.dhaug_frame_diff(a, b, 4, 9, 30, 48, 0, None) == EINVAL
    assert L.dhaug_frame_diff(a, b, 4, 9, 30, 48, 1, None) == EINVAL
    assert L.dhaug_frame_diff(a, b, 4, 9, 48, 0, 0, None) == EINVAL
    assert L.dhaug_frame_diff(a, b, -1, 9, 48, 48, 0, None) == EINVAL
    assert L.dhaug_frame_diff(None, b, 4, 9, 48, 48, 0, None) == EINVAL
    assert L.dhaug_frame_diff(None, None, 0, 9, 48, 30, 1, None) == 0
    # frame_reverse: R >= 1, w >= 1, and never in place (the rule comes after the null checks: two equal non-null addresses)
    assert L.dhaug_frame_reverse(a, a, 4, 9, 48, None) == EINVAL
    assert L.dhaug_frame_reverse(a, b, 4, 0, 48, None) == EINVAL
    assert L.dhaug_frame_reverse(a, b, 4, 9, 0, None) == EINVAL
    assert L.dhaug_frame_reverse(a, None, 4, 9, 48, None) == EINVAL
    assert L.dhaug_frame_reverse(None, None, 0, 9, 48, None) == 0
    # weighted_means: 1 .. 16 arrays, none null, none empty
    n = 17
    arrs, cnts, wts = (ctypes.c_void_p * n)(*([base] * n)), (ctypes.c_int64 * n)(*([8] * n)), (ctypes.c_float * n)(*([1.0] * n))
    assert L.dhaug_weighted_means(arrs, cnts, wts, 0, b, None) == EINVAL
    assert L.dhaug_weighted_means(arrs, cnts, wts, 17, b, None) == EINVAL
    assert L.dhaug_weighted_means(arrs, cnts, wts, -1, b, None) == EINVAL
    assert L.dhaug_weighted_means(arrs, cnts, wts, 3, None, None) == EINVAL
    cnts[1] = 0
    assert L.dhaug_weighted_means(arrs, cnts, wts, 3, b, None) == EINVAL
    cnts[1], arrs[2] = 8, None
    assert L.dhaug_weighted_means(arrs, cnts, wts, 3, b, None) == EINVAL
    # WGAN-GP rows: W in [1, 2^20], ld_bf16 >= W, B >= 0; critic_scalars: B, P, ld >= 1
    assert L.dhaug_gp_penalty(a, b, b, 4, (1 << 20) + 1, 0.25, None) == EINVAL
    assert L.dhaug_gp_penalty(a, b, b, 4, 0, 0.25, None) == EINVAL
    assert L.dhaug_gp_penalty(a, b, b, -1, 48, 0.25, None) == EINVAL
    assert L.dhaug_gp_penalty_bf16(a, b, b, 32, b, 4, 48, 0.25, None) == EINVAL
    assert L.dhaug_gp_penalty_bf16(a, b, b, 1 << 21, b, 4, (1 << 20) + 1, 0.25, None) == EINVAL
    assert L.dhaug_gp_penalty(None, None, None, 0, 48, 0.25, None) == 0
    assert L.dhaug_gp_assemble(a, a, a, b, 4, 0, None) == EINVAL
    assert L.dhaug_gp_assemble(a, a, a, b, -1, 48, None) == EINVAL
    assert L.dhaug_gp_assemble_bf16(a, a, a, b, b, 32, 4, 48, None) == EINVAL
    assert L.dhaug_gp_assemble(None, None, None, None, 0, 48, None) == 0
    assert L.dhaug_critic_scalars(a, 1, a, 0, 4, 10.0, b, b, None) == EINVAL
    assert L.dhaug_critic_scalars(a, 1, a, 4, 0, 10.0, b, b, None) == EINVAL
    assert L.dhaug_critic_scalars(a, 0, a, 4, 4, 10.0, b, b, None) == EINVAL
    assert L.dhaug_critic_scalars(a, 1, a, 4, 4, 10.0, b, None, None) == EINVAL
    # KCS: the bf16 operand's rows hold the features (ld >= W), in whole 16-byte pieces, from a 16-byte boundary
    mis = ctypes.c_void_p(base + 4096 + 2)
    assert L.dhaug_kcs_forward(a, None, b, 24, 4, 1, None) == EALIGN
    assert L.dhaug_kcs_forward(a, None, b, 8, 4, 0, None) == EALIGN
    assert L.dhaug_kcs_forward(a, None, b, 36, 4, 1, None) == EALIGN
    assert L.dhaug_kcs_forward(a, None, mis, 32, 4, 1, None) == EALIGN
    assert L.dhaug_kcs_forward(a, None, None, 0, 4, 1, None) == EINVAL                 # no output at all
    assert L.dhaug_center_kcs_forward(a, b, b, 24, 4, 1, None) == EALIGN
    assert L.dhaug_center_kcs_forward(a, None, b, 32, 4, 1, None) == EINVAL
    assert L.dhaug_d3_penalty(a, a, a, 0.5, mis, b, b, 4, None) == EALIGN
    # negative N, everywhere; N = 0 is a no-op
    for N, want in ((-1, EINVAL), (0, 0)):
        p = (lambda x: x) if N else (lambda x: None)
        assert L.dhaug_bone_length(p(a), p(b), N, None) == want
        assert L.dhaug_kcs_forward(p(a), p(b), None, 0, N, 1, None) == want
        assert L.dhaug_center_kcs_forward(p(a), p(b), p(b), 32, N, 1, None) == want
        assert L.dhaug_kcs_backward(p(a), p(a), p(b), N, 1, None) == want
        assert L.dhaug_kcs_jvp(p(a), p(a), p(b), N, 1, None) == want
        assert L.dhaug_d3_penalty(p(a), p(a), p(a), 0.5, p(b), p(b), p(b), N, None) == want
        assert L.dhaug_world_to_camera_project(p(a), p(a), p(a), p(a), p(b), p(b), N, None) == want
        assert L.dhaug_world_to_camera_project_backward(p(a), p(a), p(a), p(a), p(a), p(a), p(b), N, None) == want
        assert L.dhaug_camera_to_world(p(a), p(a), p(a), p(b), N, None) == want
        assert L.dhaug_bone_length_swap(p(a), p(a), p(b), N, None) == want
        assert L.dhaug_project_to_2d(p(a), p(a), p(b), N, None) == want
        assert L.dhaug_center_flip(p(a), p(b), N, 3, 1, 1, None) == want
        assert L.dhaug_center_flip_backward(p(a), p(b), N, 2, 1, 1, None) == want
    # camera: some output, and intrinsics whenever the projection is touched; centre / flip: C in {2, 3}
    assert L.dhaug_world_to_camera_project(a, a, a, a, None, None, 4, None) == EINVAL
    assert L.dhaug_world_to_camera_project(a, a, a, None, b, b, 4, None) == EINVAL
    assert L.dhaug_world_to_camera_project_backward(a, a, a, None, a, a, b, 4, None) == EINVAL
    assert L.dhaug_world_to_camera_project_backward(a, a, a, a, a, a, None, 4, None) == EINVAL
    for C in (0, 1, 4):
        assert L.dhaug_center_flip(a, b, 4, C, 1, 1, None) == EINVAL and L.dhaug_center_flip_backward(a, b, 4, C, 1, 1, None) == EINVAL
        assert L.dhaug_center_flip(None, None, 0, C, 1, 1, None) == EINVAL                                    # (checked before the empty batch)


def test_stream_elem_argument_errors(built):
    """the packing, column-sum, activation-backward, rank-one and Adam entry points of csrc/dhaug_elem.hip (the table of
    tests/test_gpu_stream_elem.py): every DHAUG_CHECK returns its documented code before any launch -- all pointers are HOST
    addresses, so a call that reached a launch would return a HIP error instead -- and an empty batch looks at no pointer"""
    import dhaug_amd
    L = dhaug_amd._lib.lib()
    buf = (ctypes.c_float * 8192)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a, b, c, d = (ctypes.c_void_p(base + 4096 * i) for i in range(4))
    mis2, mis8 = ctypes.c_void_p(base + 2), ctypes.c_void_p(base + 8)
    EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
    # cast_pad: (src, ld_src, dst, ld_dst, rows, cols, pad_cols)
    for args in ((a, 30, b, 32, -1, 30, 32), (a, 30, b, 32, 4, 0, 32), (a, 30, b, 32, 4, 30, 28), (a, 29, b, 32, 4, 30, 32),
                 (a, 30, b, 30, 4, 30, 32), (None, 30, b, 32, 4, 30, 32), (a, 30, None, 32, 4, 30, 32)):
        assert L.dhaug_cast_pad_bf16(*args, None) == EINVAL, args
    for args in ((a, 30, b, 32, 4, 30, 31), (a, 30, b, 33, 4, 30, 32), (a, 30, mis2, 32, 4, 30, 32)):      # odd pad_cols / ld_dst, dst % 4
        assert L.dhaug_cast_pad_bf16(*args, None) == EALIGN, args
    assert L.dhaug_cast_pad_bf16(None, 30, None, 32, 0, 30, 32, None) == 0
    # cast_transpose: rows >= 1 (no empty batch), pad_cols >= rows
    for args in ((a, 30, b, 16, 0, 30, 16), (a, 30, b, 16, 4, 0, 16), (a, 30, b, 16, 20, 30, 16), (a, 29, b, 16, 4, 30, 16),
                 (a, 30, b, 8, 4, 30, 16), (None, 30, b, 16, 4, 30, 16), (a, 30, None, 16, 4, 30, 16)):
        assert L.dhaug_cast_transpose_bf16(*args, None) == EINVAL, args
    # split_bf16: (src, ld_src, dst, rows, cols, pad_cols, mode, terms); split_f16: (..., mode)
    for args in ((a, 30, b, -1, 30, 32, 0, 3), (a, 30, b, 4, 0, 32, 0, 3), (a, 30, b, 4, 30, 24, 0, 3), (a, 29, b, 4, 30, 32, 0, 3),
                 (a, 30, b, 4, 30, 32, 3, 6), (a, 30, b, 4, 30, 32, -1, 6), (a, 30, b, 4, 30, 32, 2, 3), (a, 30, b, 4, 30, 32, 0, 4),
                 (None, 30, b, 4, 30, 32, 0, 3), (a, 30, None, 4, 30, 32, 0, 3)):
        assert L.dhaug_split_bf16(*args, None) == EINVAL, args
    for args in ((a, 30, b, 4, 30, 36, 0, 3), (a, 30, mis8, 4, 30, 32, 0, 3)):                             # pad_cols % 8, dst % 16
        assert L.dhaug_split_bf16(*args, None) == EALIGN, args
    assert L.dhaug_split_bf16(None, 30, None, 0, 30, 32, 0, 3, None) == 0
    for args in ((a, 30, b, -1, 30, 32, 0), (a, 30, b, 4, 0, 32, 0), (a, 30, b, 4, 30, 24, 0), (a, 29, b, 4, 30, 32, 0),
                 (a, 30, b, 4, 30, 32, 3), (None, 30, b, 4, 30, 32, 0), (a, 30, None, 4, 30, 32, 0)):
        assert L.dhaug_split_f16(*args, None) == EINVAL, args
    for args in ((a, 30, b, 4, 30, 36, 0), (a, 30, mis8, 4, 30, 32, 0)):
        assert L.dhaug_split_f16(*args, None) == EALIGN, args
    assert L.dhaug_split_f16(None, 30, None, 0, 30, 32, 2, None) == 0
    # repack_weights / adam_repack_step: counts in range, no null where something is to do
    assert L.dhaug_repack_weights(a, -1, None) == EINVAL and L.dhaug_repack_weights(a, 65536, None) == EINVAL
    assert L.dhaug_repack_weights(None, 3, None) == EINVAL and L.dhaug_repack_weights(None, 0, None) == 0
    rs = lambda p=a, st=b, descs=c, ndesc=2, nitems=5, w=d, nw=1: L.dhaug_adam_repack_step(p, a, a, a, 1e-4, 0.5, 0.9, 1e-8, st, 1.0, descs, ndesc,
                                                                                           nitems, w, nw, None)
    assert rs(ndesc=-1) == EINVAL and rs(nitems=-1) == EINVAL and rs(nw=-1) == EINVAL and rs(nw=65536) == EINVAL
    assert rs(st=None) == EINVAL and rs(p=None) == EINVAL and rs(descs=None) == EINVAL
    # column sums: (src, ld, dst, M, N, accumulate).  (M = 0 without accumulate clears dst on the device: tests/test_gpu_stream_elem.py)
    for fn in (L.dhaug_colsum_f32, L.dhaug_colsum_bf16):
        for args in ((a, 8, b, -1, 8, 1), (a, 8, b, 4, 0, 1), (a, 7, b, 4, 8, 1), (a, 8, None, 4, 8, 1), (None, 8, b, 4, 8, 1)):
            assert fn(*args, None) == EINVAL, args
        assert fn(None, 8, b, 0, 8, 1, None) == 0
    # act_backward_bf16: (g, ld_g, y, ld_y, dst, ld_dst, M, N, act, slope)
    for args in ((a, 16, b, 16, c, 16, -1, 16, 1, 0.0), (a, 16, b, 16, c, 16, 4, 0, 1, 0.0), (a, 16, b, 16, c, 16, 4, 7, 1, 0.0),
                 (a, 16, b, 16, c, 16, 4, 16, 3, 0.0), (a, 16, b, 16, c, 16, 4, 16, -1, 0.0), (None, 16, b, 16, c, 16, 4, 16, 1, 0.0),
                 (a, 16, None, 16, c, 16, 4, 16, 1, 0.0), (a, 16, b, 16, None, 16, 4, 16, 1, 0.0)):
        assert L.dhaug_act_backward_bf16(*args, None) == EINVAL, args
    for args in ((a, 16, b, 16, c, 16, 4, 12, 1, 0.0), (a, 20, b, 16, c, 16, 4, 16, 1, 0.0), (a, 16, b, 20, c, 16, 4, 16, 1, 0.0),
                 (a, 16, b, 16, c, 20, 4, 16, 1, 0.0), (mis2, 16, b, 16, c, 16, 4, 16, 1, 0.0), (a, 16, mis8, 16, c, 16, 4, 16, 1, 0.0),
                 (a, 16, b, 16, mis8, 16, 4, 16, 1, 0.0)):
        assert L.dhaug_act_backward_bf16(*args, None) == EALIGN, args
    assert L.dhaug_act_backward_bf16(None, 16, None, 16, None, 16, 0, 16, 1, 0.0, None) == 0
    for args in ((a, b, c, -1, 1, 0.0), (a, b, c, 4, 3, 0.0), (a, b, c, 4, -1, 0.0), (None, b, c, 4, 1, 0.0), (a, None, c, 4, 1, 0.0),
                 (a, b, None, 4, 1, 0.0)):
        assert L.dhaug_act_backward_f32(*args, None) == EINVAL, args
    assert L.dhaug_act_backward_f32(None, None, None, 0, 2, 0.1, None) == 0
    for args in ((a, b, c, -1), (None, b, c, 4), (a, None, c, 4), (a, b, None, 4)):
        assert L.dhaug_add_f32(*args, None) == EINVAL, args
    assert L.dhaug_add_f32(None, None, None, 0, None) == 0
    # Adam: (p, g, m, v, n, lr, b1, b2, eps, step | step_dev, grad_scale); step >= 1
    hp = (1e-4, 0.5, 0.9, 1e-8)
    for ptrs, n, step in (((a, b, c, d), -1, 1), ((a, b, c, d), 4, 0), ((a, b, c, d), 4, -3), ((a, b, c, d), 0, 0), ((None, b, c, d), 4, 1),
                          ((a, None, c, d), 4, 1), ((a, b, None, d), 4, 1), ((a, b, c, None), 4, 1)):
        assert L.dhaug_adam_step(*ptrs, n, *hp, step, 1.0, None) == EINVAL, (n, step)
    assert L.dhaug_adam_step(None, None, None, None, 0, *hp, 1, 1.0, None) == 0
    for ptrs, n, cnt in (((a, b, c, d), -1, a), ((None, b, c, d), 4, a), ((a, None, c, d), 4, a), ((a, b, None, d), 4, a),
                         ((a, b, c, None), 4, a), ((a, b, c, d), 4, None)):
        assert L.dhaug_adam_step_dev(*ptrs, n, *hp, cnt, 1.0, None) == EINVAL, n
    assert L.dhaug_adam_step_dev(None, None, None, None, 0, *hp, None, 1.0, None) == 0
    assert L.dhaug_counter_add(None, 1, None) == EINVAL
    # rank1_mask: (seed, ld_seed, w, ld_w, mask, ld_mask, out, ld_out, M, N, pad_cols, mask_act, mask_slope)
    for args in ((a, 1, b, 1, c, 112, d, 112, -1, 100, 112, 1, 0.0), (a, 1, b, 1, c, 112, d, 112, 4, 0, 112, 1, 0.0),
                 (a, 1, b, 1, c, 112, d, 112, 4, 100, 96, 1, 0.0), (a, 1, b, 1, c, 112, d, 112, 4, 100, 100, 1, 0.0),
                 (a, 1, b, 1, c, 112, d, 112, 4, 100, 112, 0, 0.0), (a, 1, b, 1, c, 112, d, 112, 4, 100, 112, 3, 0.0),
                 (None, 1, b, 1, c, 112, d, 112, 4, 100, 112, 1, 0.0), (a, 1, None, 1, c, 112, d, 112, 4, 100, 112, 1, 0.0),
                 (a, 1, b, 1, None, 112, d, 112, 4, 100, 112, 1, 0.0), (a, 1, b, 1, c, 112, None, 112, 4, 100, 112, 1, 0.0)):
        assert L.dhaug_rank1_mask_bf16(*args, None) == EINVAL, args
    assert L.dhaug_rank1_mask_bf16(a, 1, b, 1, c, 1032, d, 1032, 4, 1025, 1032, 1, 0.0, None) == EUNSUPPORTED     # pad_cols > 1 024
    for args in ((a, 0, b, 1, c, 112, d, 112, 4, 100, 112, 1, 0.0), (a, 1, b, 0, c, 112, d, 112, 4, 100, 112, 1, 0.0),
                 (a, 1, b, 1, c, 104, d, 112, 4, 100, 112, 1, 0.0), (a, 1, b, 1, c, 112, d, 104, 4, 100, 112, 1, 0.0),
                 (a, 1, b, 1, c, 116, d, 112, 4, 100, 112, 1, 0.0), (a, 1, b, 1, c, 112, d, 116, 4, 100, 112, 1, 0.0),
                 (a, 1, b, 1, mis8, 112, d, 112, 4, 100, 112, 1, 0.0), (a, 1, b, 1, c, 112, mis8, 112, 4, 100, 112, 1, 0.0)):
        assert L.dhaug_rank1_mask_bf16(*args, None) == EALIGN, args
    assert L.dhaug_rank1_mask_bf16(None, 1, None, 1, None, 112, None, 112, 0, 100, 112, 1, 0.0, None) == 0
    # rank1_bits: (seed, ld_seed, w, ld_w, bits, out, ld_out, M, mask_act, mask_slope)
    for args in ((a, 1, b, 1, c, d, 256, -1, 1, 0.0), (a, 1, b, 1, c, d, 256, 4, 0, 0.0), (None, 1, b, 1, c, d, 256, 4, 1, 0.0),
                 (a, 1, None, 1, c, d, 256, 4, 1, 0.0), (a, 1, b, 1, None, d, 256, 4, 1, 0.0), (a, 1, b, 1, c, None, 256, 4, 1, 0.0)):
        assert L.dhaug_rank1_bits_bf16(*args, None) == EINVAL, args
    for args in ((a, 0, b, 1, c, d, 256, 4, 1, 0.0), (a, 1, b, 0, c, d, 256, 4, 1, 0.0), (a, 1, b, 1, c, d, 248, 4, 1, 0.0),
                 (a, 1, b, 1, c, d, 260, 4, 1, 0.0), (a, 1, b, 1, mis8, d, 256, 4, 1, 0.0), (a, 1, b, 1, c, mis8, 256, 4, 1, 0.0)):
        assert L.dhaug_rank1_bits_bf16(*args, None) == EALIGN, args
    assert L.dhaug_rank1_bits_bf16(None, 1, None, 1, None, None, 256, 0, 2, 0.2, None) == 0


def test_stream_elem_references_reject_emulated_faults():
    """tests/stream_elem_util.py on the host, at small sizes: its references accept a faithful emulation of each kernel's output and
    the comparisons of tests/test_gpu_stream_elem.py reject the faults a streaming kernel can have -- the last row dropped, the tail
    chunk of a row left unwritten, one element written past the pad, the second trip of a capped loop skipped (out of place, in
    place, and in Adam), the column-sum fold pairing r with r + 1"""
    import stream_elem_util as S
    BF16 = torch.bfloat16
    payload = S.bf16_from_bits([S.PAYLOAD16])[0]

    def emulate(ref, ld):
        """a payload-filled (rows, ld) output that a faithful kernel wrote ref into"""
        out = payload.repeat(ref.shape[0], ld)
        out[:, :ref.shape[1]] = ref
        return out

    x = S.special_matrix(9, 30, S.SPECIAL_F32, seed=1)
    cases = [("cast_pad", S.cast_pad_ref(x, 32)), ("cast_transpose", S.cast_transpose_ref(x, 16)),
             ("split_bf16 (1, 6)", S.split_ref(x, S.SPLIT_BF16_LAYOUT[(1, 6)], 32, False)),
             ("split_f16 2", S.split_ref(S.special_matrix(9, 30, S.SPECIAL_F16_SAFE, seed=2), S.SPLIT_F16_LAYOUT[2], 32, True))]
    g = S.gen(3)
    gv, yv = torch.randn(9, 32, generator=g).to(BF16), S.plant_mask(torch.randn(9, 32, generator=g).to(BF16), seed=4)
    cases.append(("act_backward", S.act_backward_ref(gv, yv, 2, 0.01)))
    sd, w = torch.randn(9, generator=g).to(BF16), torch.randn(30, generator=g).to(BF16)
    cases.append(("rank1", S.rank1_ref(sd, w, yv, 30, 32, 0.2)))
    for name, ref in cases:
        ref = ref.view(BF16) if ref.dtype != BF16 else ref                # (16-bit patterns: the comparison is on bits)
        width = ref.shape[1]
        good = emulate(ref, width + 8)
        assert S.rows_ok(good, width, ref, nan_ok=True), name
        bad = good.clone(); bad[-1] = payload                             # the last row dropped
        assert not S.rows_ok(bad, width, ref, nan_ok=True), name
        bad = good.clone(); bad[:, width - 8:width] = payload             # the tail chunk of every row left unwritten
        assert not S.rows_ok(bad, width, ref, nan_ok=True), name
        bad = good.clone(); bad[-1, width - 8:width] = payload            # ... of the last row only
        assert not S.rows_ok(bad, width, ref, nan_ok=True), name
        bad = good.clone(); bad[4, width] = 0.0                           # one element past the pad written (a zero, as a pad would be)
        assert not S.rows_ok(bad, width, ref, nan_ok=True), name
        flat = good.clone()                                               # the second trip skipped: items beyond the first 2/3 untouched
        flat[6:] = payload
        assert not S.rows_ok(flat, width, ref, nan_ok=True), name
    # a pad column that holds data instead of zeros, a duplicated segment that differs
    ref = S.split_ref(x, S.SPLIT_BF16_LAYOUT[(0, 3)], 32, False)
    bad = ref.clone(); bad[:, 31] = bad[:, 29]
    assert not S.rows_ok(bad, 96, ref) and S.rows_ok(ref.clone(), 96, ref, nan_ok=True)
    # in place, the second trip skipped: the skipped rows still hold g, which differs from g * act'(y) wherever y <= 0
    for act in (1, 2):
        ref = S.act_backward_ref(gv, yv, act, 0.01)
        stale = ref.clone(); stale[6:] = gv[6:]
        assert S.rows_ok(ref.clone(), 32, ref) and not S.rows_ok(stale, 32, ref), act
    # the bit compare of rank1_mask against the float compare: a signed 16-bit compare would differ only on NaN masks; a compare that
    # took -0 or a negative subnormal for positive is rejected by the planted values
    wrong = torch.where(S.ibits(yv) != 0, gv.float(), gv.float() * 0.01).to(BF16)
    assert not S.rows_ok(wrong, 32, S.act_backward_ref(gv, yv, 2, 0.01))
    # column sums: a dropped row; the fold
    xi = S.int_matrix(65, 9, seed=5)
    assert S.exact_sums_ok(xi.sum(0), xi) and not S.exact_sums_ok(xi[:-1].sum(0), xi)
    y = S.folded(torch.randn(72, 64, generator=S.gen(6)))
    assert float(S.colsum_emulate(y, lambda r, h: r + h).abs().max()) == 0.0               # the kernel's pairing: exactly zero
    assert float(S.colsum_emulate(y, lambda r, h: r + 1).abs().max()) > 0.0                # r with r + 1: it is not
    # Adam at two small sizes: the fp32 restatement passes its own rule; one skipped element, a skipped tail and a missing
    # grad_scale do not; the multi-pass size and its bounds are checked here too (the condition bound(p) < lr / 10)
    for n in (257, 1000):
        c = S.adam_case(n)
        assert S.adam_check("ref32 n=%d" % n, c["ref32"], c)[0] < S.ADAM_LR / 10
        one = c["ref32"][0].clone(); one[n // 2] = c["p0"][n // 2]
        tail = c["ref32"][0].clone(); tail[256:] = c["p0"][256:]
        for bad in (one, tail):
            with pytest.raises(AssertionError):
                S.adam_check("faulty", (bad, c["ref32"][1], c["ref32"][2]), c)
        p, m, v = c["p0"], torch.zeros(n), torch.zeros(n)
        for step, gr in zip(S.ADAM_STEPS, c["grads"]):
            p, m, v = S.adam_ref(p, gr, m, v, step, torch.float32, gscale=1.0)
        with pytest.raises(AssertionError):
            S.adam_check("no grad_scale", (p, m, v), c)
        z = S.ADAM_ZERO_AT
        assert S.ibits(c["ref32"][0])[z] == S.ibits(c["p0"])[z]                              # g = m = v = 0 keeps the parameter's bits
    for kernel in ("cast_pad", "cast_transpose", "split", "act_bf16", "rank1", "flat", "adam_nt"):
        n, per = S.items(kernel)
        assert per < n < 2 * per, kernel                                                    # exactly one more, partial, trip


def test_parity_program_planner_refuses_what_one_image_cannot_hold(built):
    """dhaug_mlp_forward_x3 plans the three virtual buffers of a program onto ONE in-place LDS image (+ registers + a workspace)
    on the host, before any launch: a program that reads a value from where it no longer is comes back DHAUG_EUNSUPPORTED, mixed
    fragment layouts and a parked result without a workspace DHAUG_EINVAL -- checked here without a GPU."""
    import dhaug_amd
    from dhaug_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ptr = ctypes.c_void_p(base)

    def unit(kind, **kw):
        u = _lib.MlpUnit()
        u.kind, u.src, u.dst, u.res, u.src2 = kind, -1, -1, -1, -1
        for k, v in kw.items():
            setattr(u, k, v)
        return u

    def run(units):
        arr = (_lib.MlpUnit * len(units))(*units)
        return L.dhaug_mlp_forward_x3(arr, len(units), 128, None)

    LOAD, GEMM, OUT, T16 = 0, 3, 4, 32
    load = lambda dst: unit(LOAD, dst=dst, cols=64, ld=64, g=ptr)
    gemm = lambda src, dst, **kw: unit(GEMM, src=src, dst=dst, ksteps=4, n=256, w=ptr, bias=ptr, **kw)
    # the source must be what the image holds: buffer 0 was never written
    assert run([load(1), gemm(0, 1)]) == -3
    # buffer 1 is read again as a SOURCE after the layer in between has overwritten the image
    assert run([load(1), gemm(1, 0), gemm(1, 0)]) == -3
    # one fragment layout per program
    assert run([load(1), gemm(1, 0, flags=T16), gemm(0, 1)]) == -1
    # a result that waits while another branch uses the image needs the workspace (g of the GEMM units that are not outputs)
    parked = [load(1), gemm(1, 0), unit(GEMM, src=0, dst=2, ksteps=16, n=100, w=ptr, bias=ptr), load(1), gemm(1, 0),
              unit(GEMM, src=0, dst=2, res=2, ksteps=16, n=100, w=ptr, bias=ptr)]
    assert run(parked) == -1
    # a second source (a concatenation in one unit) is not a unit of this kernel
    assert run([load(1), unit(GEMM, src=1, dst=0, src2=0, ksteps2=4, ksteps=4, n=256, w=ptr, w2=ptr, bias=ptr)]) == -3
    assert run([]) == -1


def test_ops_refuse_cpu_tensors(built):
    from dhaug_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fk_forward(torch.zeros(2, 37), torch.zeros(2, 15), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kcs_forward(torch.zeros(2, 16, 3))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "dh-aug-dh-forward-kinematics-model-driven-augmentation-for-3d-human-pose-estimation_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                assert "oracle" not in src, os.path.join(d, f)


def test_environment_switches_are_documented():
    """every DHAUG_* variable the package's Python modules read has a row in INTEGRATION.md's table, and the retired switches
    (spelt here without their prefix, so that this file passes its own scan) are named by no source file any more"""
    pkg = os.path.join(ROOT, "dh-aug-dh-forward-kinematics-model-driven-augmentation-for-3d-human-pose-estimation_amd")
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    read = set()
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                read |= set(re.findall(r"environ\.get\(\s*[\"'](DHAUG_[A-Z0-9_]+)[\"']", open(os.path.join(d, f)).read()))
    assert len(read) >= 20 and "DHAUG_NO_TN_SPLIT" in read, sorted(read)      # (the scan found the reads)
    missing = sorted(n for n in read if not re.search(r"\| `%s` \|" % n, doc))
    assert not missing, "INTEGRATION.md's switch table does not list %s" % missing
    retired = ["DHAUG_" + n for n in ("TN_PHASED", "TN_MAIN_WGS", "PARTITION", "CU_SHARES", "NO_TN_GROUP", "NO_RANK1", "NO_SPLIT_CACHE",
                                      "NO_BLOCK2_STACK", "NO_DBITS", "NO_SIGN_BITS")]
    pat = re.compile(r"\b(%s)\b" % "|".join(retired))
    tops = [pkg] + [os.path.join(ROOT, t) for t in ("include", "tests", "tools", "oracle")]
    paths = [os.path.join(ROOT, f) for f in os.listdir(ROOT)]
    for t in tops:
        for d, dirs, files in os.walk(t):
            dirs[:] = [x for x in dirs if x not in ("_ref", "_build", "__pycache__")]      # (built, not source)
            paths += [os.path.join(d, f) for f in files]
    n = 0
    for p in paths:
        if p.endswith((".py", ".hip", ".h", ".sh")) and os.path.isfile(p):
            n += 1
            hit = pat.search(open(p, errors="replace").read())
            assert hit is None, "%s still names %s" % (p, hit.group(1))
    assert n > 100


def test_module_state_dict_keys_and_host_logic(built):
    """module construction, state_dict key parity with the reference, config defaults: all host-side"""
    import golden_util as GU
    from dhaug_amd.function_aug.config import get_parse_args
    from dhaug_amd.models_Fk_GAN import Fk_discriminator as dis, Fk_generator as gen, forward_kinematics_DH_model as fkm
    from dhaug_amd.models_Fk_GAN.video_mode_operate import video_receptive_field
    args = get_parse_args([])
    assert args.batch_size == 1024 and args.GAN_OUTPUT_DIM == 35 and args.GAN_LAMBDA == 10 and args.Gen_DenseDim == 1000
    assert args.bone_len_scaler == "different" and args.flip_GAN_model_input is True and args.architecture == "3,3,3"
    a2 = get_parse_args(["--batch_size", "512", "--GAN_whether_use_preAngle", "False", "--architecture", "3,3",
                         "--single_or_multi_train_mode", "multi"])
    assert a2.batch_size == 512 and a2.GAN_whether_use_preAngle is False
    assert video_receptive_field([3, 3]) == 9 and video_receptive_field([3, 3, 3]) == 27
    args.Gen_DenseDim = args.Dis_DenseDim_3D = args.Dis_DenseDim_2D = 32
    fk = fkm.Forward_Kinematics_DH_Model(args, ["S1"], None)
    G = gen.Fk_Generator(fk, args, "cpu")
    assert list(G.state_dict().keys()) == list(GU.shapes_generator(32).keys())
    assert {k: tuple(v.shape) for k, v in G.state_dict().items()} == GU.shapes_generator(32)
    D3 = dis.Fk_3D_Discriminator("cpu", args)
    assert {k: tuple(v.shape) for k, v in D3.state_dict().items()} == GU.shapes_d3(32)
    D2 = dis.Fk_2D_Discriminator(args, 16)
    assert {k: tuple(v.shape) for k, v in D2.state_dict().items()} == GU.shapes_d2(32)
    assert sum(p.numel() for p in gen.Fk_Generator(fk, get_parse_args(["--Gen_DenseDim", "256"]), "cpu").parameters()) == 436771
    assert fkm.H36M_32_To_16_Table == [0, 1, 2, 3, 6, 7, 8, 12, 13, 15, 17, 18, 19, 25, 26, 27]


def test_hostcheck_fk_math_matches_oracle(built):
    """the per-pose arithmetic of csrc/dhaug_fk_math.h, compiled for the HOST by the test-only harness, against
    the oracle: forward <= 1e-5 abs, reverse mode <= 1e-4 relative (the device runs the same source)."""
    import numpy as np
    import golden_util as GU
    from oracle import dhaug_oracle as O
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hostcheck", "_build", "libhostcheck.so"))
    P = ctypes.POINTER(ctypes.c_float)
    ptr = lambda a: a.ctypes.data_as(P)
    N = 2048
    a, bl, rt = GU.synth_fk_inputs(N, 3)
    an, bn, rn = a.numpy().copy(), bl.numpy().copy(), rt.numpy().copy()
    out = np.zeros((N, 48), np.float32)
    lib.hostcheck_fk_forward(ptr(an), ptr(bn), ptr(rn), ptr(out), ctypes.c_long(N))
    assert np.abs(out - O.fk_forward16(a, bl, rt).reshape(N, 48).numpy()).max() <= 1e-5
    g = torch.randn(N, 16, 3, generator=torch.Generator().manual_seed(1))
    ad, bd, rd = (t.double().requires_grad_(True) for t in (a, bl, rt))
    (O.fk_forward16(ad, bd, rd) * g.double()).sum().backward()
    ga, gb, gr = np.zeros((N, 37), np.float32), np.zeros((N, 15), np.float32), np.zeros((N, 3), np.float32)
    gn = g.numpy().reshape(N, 48).copy()
    lib.hostcheck_fk_backward(ptr(an), ptr(bn), ptr(gn), ptr(ga), ptr(gb), ptr(gr), ctypes.c_long(N))
    for got, ref in ((ga, ad.grad), (gb, bd.grad), (gr, rd.grad)):
        assert np.abs(got - ref.numpy()).max() <= 1e-4 * ref.abs().max().item()


# (M, N, K, what differs from the defaults, kernel, KSTEPS / KS).  Defaults: bf16 output only, no fp32 residual, no fp32 mask, bias
# aligned, W = N, p8_ok, no switch set.  Derived by hand from the dispatcher as it was before the routing became a function of its own.
NT_ROUTES = [
    (4096, 256, 256, {}, "NT256S", 16),
    (4096, 256, 128, {}, "NT256S", 8),
    (4128, 256, 256, {}, "WS", 16),                                  # M % 64 != 0
    (4096, 256, 256, {"out_f32": 1}, "WS", 16),
    (4096, 256, 256, {"res_f32": 1}, "WS", 16),
    (4096, 256, 256, {"bias_ok": 0}, "WS", 16),
    (4096, 256, 256, {"no256": 1}, "WS", 16),
    (4096, 256, 64, {}, "WS", 4),
    (4096, 256, 112, {}, "WS", 7),
    (4096, 256, 80, {}, "PIPE2", 0),
    (4096, 256, 96, {}, "PIPE2", 0),
    (4096, 256, 272, {}, "PIPE2", 0),
    (4096, 65, 16, {}, "WS", 1),
    (4096, 60, 256, {"W": 128}, "WS", 16),                           # zero-padded output
    (4096, 64, 256, {}, "GENERIC_128x64", 0),
    (4096, 33, 256, {}, "GENERIC_128x64", 0),
    (4096, 32, 256, {}, "GENERIC_128x32", 0),
    (4096, 512, 256, {}, "WS", 16),                                  # ws precedes big
    (4096, 512, 272, {}, "BIG", 0),
    (4096, 1000, 1008, {}, "BIG", 0),
    (4095, 1000, 1008, {}, "PIPE2", 0),
    (13824, 1000, 1008, {}, "P8", 0),
    (13824, 1000, 1008, {"nop8": 1}, "WIDE", 0),
    (13824, 1000, 1008, {"p8_ok": 0}, "WIDE", 0),
    (13824, 1000, 1008, {"nobig": 1}, "PIPE2", 0),
    (40960, 256, 768, {}, "P8", 0),                                  # 160 tiles
    (40704, 256, 768, {}, "PIPE2", 0),                               # 159 tiles, W < 512
    (40705, 256, 768, {}, "P8", 0),                                  # the ceiling gives 160
    (512, 256, 768, {"wide_min_tiles": 1}, "P8", 0),
    (4096, 256, 256, {"mask_f32": 1, "out_bf16": 0, "out_f32": 1}, "PIPE2", 0),
    (4096, 256, 48, {"mask_f32": 1, "out_bf16": 0, "out_f32": 1}, "GENERIC_128x128", 0),
    (4096, 64, 48, {"mask_f32": 1, "out_bf16": 0, "out_f32": 1}, "GENERIC_128x64", 0),
]
TN_ROUTES = [
    (4096, 256, 256, "TN64"), (512, 64, 64, "TN64"), (384, 64, 64, "TN_GENERIC"), (1920, 64, 128, "TN64"),
    (1920, 100, 100, "TN_GENERIC"), (6144, 100, 100, "TN64"), (12288, 1, 100, "TN64"), (1000, 100, 512, "TN_GENERIC"),
    (65728, 128, 384, "TN_GENERIC"),
]


def test_gemm_routes(built):
    """which kernel the NT and TN dispatchers of csrc/dhaug_gemm.hip take for a shape: csrc/dhaug_gemm_route.h, the very functions
    the dispatchers call, compiled for the host."""
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hostcheck", "_build", "libhostcheck.so"))
    LL = ctypes.c_longlong
    lib.hostcheck_nt_route.argtypes = [LL] * 4 + [ctypes.c_int] * 9 + [LL]
    lib.hostcheck_tn_route.argtypes = [LL] * 3
    nt_names = ["NT256S", "WS", "P8", "WIDE", "BIG", "PIPE2", "GENERIC_128x128", "GENERIC_128x64", "GENERIC_128x32"]   # enum NtKernel
    tn_names = ["TN64", "TN_GENERIC"]                                                                                   # enum TnKernel
    bad = []
    for M, N, K, extra, kernel, ks in NT_ROUTES:
        a = dict(W=N, out_bf16=1, out_f32=0, res_f32=0, bias_ok=1, mask_f32=0, p8_ok=1, no256=0, nobig=0, nop8=0, wide_min_tiles=-1)
        assert set(extra) <= set(a)
        a.update(extra)
        r = lib.hostcheck_nt_route(M, N, a["W"], K, a["out_bf16"], a["out_f32"], a["res_f32"], a["bias_ok"], a["mask_f32"], a["p8_ok"],
                                   a["no256"], a["nobig"], a["nop8"], a["wide_min_tiles"])
        got = (nt_names[r // 100], r % 100)
        if got != (kernel, ks):
            bad.append(((M, N, K, extra), got, (kernel, ks)))
    for M, N1, N2, kernel in TN_ROUTES:
        got = tn_names[lib.hostcheck_tn_route(M, N1, N2)]
        if got != kernel:
            bad.append(((M, N1, N2), got, kernel))
    assert not bad, bad


def test_gemm_case_table_reaches_every_route(built):
    """tests/gemm_cases.py means what it says: every record of the table tests/test_gpu_gemm_routes.py runs is routed, by the very
    functions the dispatchers call, to the kernel and KSTEPS it names (a record whose route does not read dhaug_p8_supported() gets
    the same answer for either value), and the table as a whole reaches every NT kernel, every instantiation of the two templated
    ones, and both TN kernels."""
    import gemm_cases as G
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "hostcheck", "_build", "libhostcheck.so"))
    LL = ctypes.c_longlong
    lib.hostcheck_nt_route.argtypes = [LL] * 4 + [ctypes.c_int] * 9 + [LL]
    lib.hostcheck_tn_route.argtypes = [LL] * 3
    bad, seen_nt, seen_tn = [], set(), set()
    for c in G.NT_CASES:
        assert set(k for k, _ in c.env) <= set(G.SWITCHES)
        for p8_ok in ((False, True) if c.p8_ok is None else (c.p8_ok,)):
            r = lib.hostcheck_nt_route(*c.route_args(p8_ok))
            got = (G.NT_KERNELS[r // 100], r % 100)
            if got != (c.kernel, c.ksteps):
                bad.append((c.ident, p8_ok, got))
        seen_nt.add((c.kernel, c.ksteps))
    for c in G.TN_CASES:
        got = G.TN_KERNELS[lib.hostcheck_tn_route(c.M, c.N1, c.N2)]
        if got != c.kernel:
            bad.append((c.ident, got))
        seen_tn.add(c.kernel)
    assert not bad, bad
    assert set(k for k, _ in seen_nt) == set(G.NT_KERNELS) and len(G.NT_KERNELS) == 9
    assert set(ks for k, ks in seen_nt if k == "WS") == set(G.WS_KSTEPS) == {1, 2, 3, 4, 7, 8, 16}
    assert set(ks for k, ks in seen_nt if k == "NT256S") == set(G.NT256S_KSTEPS) == {8, 16}
    assert seen_tn == set(G.TN_KERNELS) and len(G.TN_KERNELS) == 2


def test_hostcheck_under_address_and_ub_sanitizers(built, tmp_path):
    """the same host build as an executable under -fsanitize=address,undefined (-fno-sanitize-recover): ordinary poses and
    the degenerate ones of tests/test_gpu_edge.py (angles of +-1e4 and +-1e7 degrees -- the library path of the range
    reduction --, zero bone lengths, inf / NaN angles) run clean, and the ordinary poses still match the oracle."""
    import subprocess
    import numpy as np
    import golden_util as GU
    from oracle import dhaug_oracle as O
    import __graft_entry__ as ge
    exe = ge.build_hostcheck_sanitized(verbose=False)
    N = 512
    a, bl, rt = GU.synth_fk_inputs(N, 17)
    a, bl = a.clone(), bl.clone()
    a[256:320] *= 55.0                      # +-1e4 deg
    a[320:384] *= 5.0e4                     # +-1e7 deg: beyond the Cody-Waite window
    bl[384:400] = 0.0
    a[400, 3] = float("inf"); a[401, 12] = float("nan"); a[402, 36] = -float("inf")
    g = torch.randn(N, 48, generator=torch.Generator().manual_seed(2))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.int64(N).tobytes())
        for t in (a, bl, rt, g):
            f.write(t.numpy().astype(np.float32).tobytes())
    r = subprocess.run([exe, str(fin), str(fout)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out = np.fromfile(fout, dtype=np.float32)[:N * 48].reshape(N, 48)
    ref = O.fk_forward16(a, bl, rt).reshape(N, 48).numpy()
    ok = np.r_[0:400]
    assert np.abs(out[ok] - ref[ok]).max() <= 1e-5
