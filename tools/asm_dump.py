#!/usr/bin/env python3
"""Device assembly of every libadayolo.so source of a tree, one .s per file: asm_dump.py TREE OUTDIR [-- extra hipcc flags]
Two trees whose device code is the same give identical directories (`diff -r A B`): -fuse-cuid=none keeps the per-compile
__hip_cuid symbol out of the text. The sources and flags are read from TREE's own adaptiveisp_amd/build.py."""
import importlib.util, os, subprocess, sys
from concurrent.futures import ThreadPoolExecutor
args = sys.argv[1:]
extra = args[args.index("--") + 1:] if "--" in args else []
tree, out = [os.path.abspath(a) for a in (args[:args.index("--")] if "--" in args else args)]
spec = importlib.util.spec_from_file_location("tree_build", os.path.join(tree, "adaptiveisp_amd", "build.py"))
b = importlib.util.module_from_spec(spec)
spec.loader.exec_module(b)
lib = b.LIBS["libadayolo.so"]
os.makedirs(out, exist_ok=True)


def one(s):
    # cwd = the tree's csrc and a relative source name, so that no path of the tree reaches the text
    r = subprocess.run([b._hipcc(), f"--offload-arch={b.ARCH}", *lib["flags"], *extra, "-S", "--cuda-device-only", "-fuse-cuid=none",
                        s, "-o", os.path.join(out, s.rsplit(".", 1)[0] + ".s")], cwd=b.CSRC, capture_output=True, text=True)
    return s, r.returncode, r.stderr


with ThreadPoolExecutor(max_workers=6) as ex:
    bad = [(s, err) for s, rc, err in ex.map(one, lib["sources"]) if rc]
for s, err in bad:
    print(f"{s}: hipcc failed\n{err[-3000:]}")
sys.exit(1 if bad else 0)
