#!/usr/bin/env python3
"""Is a source file's device code the same as at an earlier revision?

    python tools/same_isa.py <csrc file> [<git rev>, default HEAD~1]

Compiles the working-tree file and the file as it was at <rev> (with that revision's headers) to device assembly with the
flags the build gives that file, drops comments, debug directives and the per-source __hip_cuid_ symbol, and diffs the
rest; prints both sides' per-kernel resource usage.  Exit status 0: identical, 1: not."""
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import CSRC, HIPCC, HIP_FLAGS, per_file_flags  # noqa: E402

DROP = re.compile(r"\s*(;|//|\.file\b|\.loc\b|\.ident\b)|.*__hip_cuid_")


def device_asm(src, root):
    """(assembly lines, resource remarks) of `src`, headers taken from the tree at `root`"""
    flags = [f.replace(ROOT, root) if f.startswith("-I") else f for f in HIP_FLAGS] + per_file_flags(src)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "dev.s")
        r = subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", out],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.exit("compile failed: %s\n%s" % (src, r.stdout))
        asm = [ln for ln in open(out).read().splitlines() if not DROP.match(ln)]
    return asm, [ln.split("remark: ", 1)[1].split(" [-R")[0] for ln in r.stdout.splitlines() if "remark: " in ln]


def main():
    src = os.path.abspath(sys.argv[1])
    rev = sys.argv[2] if len(sys.argv) > 2 else "HEAD~1"
    rel = os.path.relpath(src, ROOT)
    with tempfile.TemporaryDirectory() as old:
        tracked = subprocess.check_output(["git", "-C", ROOT, "ls-tree", "-r", "--name-only", rev, os.path.relpath(CSRC, ROOT),
                                           "include/dhaug.h"], text=True).splitlines()
        for f in tracked:                            # (all of csrc/: a source may include another)
            os.makedirs(os.path.dirname(os.path.join(old, f)), exist_ok=True)
            with open(os.path.join(old, f), "wb") as fh:
                fh.write(subprocess.check_output(["git", "-C", ROOT, "show", "%s:%s" % (rev, f)]))
        with concurrent.futures.ThreadPoolExecutor(2) as ex:
            new, was = ex.submit(device_asm, src, ROOT), ex.submit(device_asm, os.path.join(old, rel), old)
            (new_asm, new_res), (old_asm, old_res) = new.result(), was.result()
    for name, res in ((rev, old_res), ("working tree", new_res)):
        print("== resource usage, %s\n%s" % (name, "\n".join(res)))
    diff = list(difflib.unified_diff(old_asm, new_asm, rev, "working tree", lineterm="", n=2))
    print("\n".join(diff[:200]))
    same = not diff and old_res == new_res
    print("device code: %s (%d lines compared)" % ("IDENTICAL" if same else "DIFFERENT", len(new_asm)))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
