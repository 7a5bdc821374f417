#!/usr/bin/env python3
"""Device assembly of every libadayolo.so source of a tree, one .s per file: asm_dump.py TREE OUTDIR [-- extra hipcc flags]
Two trees whose device code is the same give identical directories (`diff -r A B`): -fuse-cuid=none keeps the per-compile
__hip_cuid symbol out of the text. The sources and flags are read from TREE's own adaptiveisp_amd/build.py.

asm_dump.py --tables OUTDIR_A OUTDIR_B [file.s ...]: for every kernel of two dumps, the resources (vgpr, agpr, sgpr, vgpr / sgpr
spills, scratch bytes, LDS bytes), the instruction count, and whether the ordered list of its MFMAs, LDS-DMA loads, barriers and
counted vmcnt waits (the k-loop's structure and DMA schedule) is the same. Exit code 1 if any resource or list differs."""
import importlib.util, os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor

RES = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
       "group_segment_fixed_size"]
SCHED = re.compile(r"^\t(v_mfma\S*|global_load_lds\S*|buffer_load\S*(?=.*\blds\b)|s_barrier\b|s_waitcnt(?=.*vmcnt\(\d+\)))")


def kernels(path):
    """{kernel symbol: (resources, instruction count, schedule list)} of one .s file"""
    text = open(path).read().split("\n")
    meta, rec = {}, None
    for ln in text:                                       # amdhsa.kernels: one "  - .field:" record per kernel, fields in name order
        m = re.match(r"^  (- |  )\.(\w+):\s+(\S+)", ln)
        if m and m.group(1) == "- ":
            rec = {}
        if m and rec is not None:
            if m.group(2) in RES:
                rec[m.group(2)] = int(m.group(3))
            elif m.group(2) == "symbol":
                meta[m.group(3)[:-3]] = rec
    out, cur = {}, None
    for ln in text:
        m = re.match(r"^(\w+):", ln)
        if m and m.group(1) in meta:
            cur = m.group(1)
            out[cur] = (meta[cur], 0, [])
        elif cur and ln.startswith(".Lfunc_end"):     # (not s_endpgm: a kernel with early returns has several)
            cur = None
        elif cur and re.match(r"^\t[a-z]", ln):
            res, n, sched = out[cur]
            m = SCHED.match(ln)
            if m:
                w = re.search(r"vmcnt\(\d+\)", ln)
                sched.append(w.group(0) if m.group(1) == "s_waitcnt" else m.group(1))
            out[cur] = (res, n + 1, sched)
    return out


def tables(da, db, files):
    files = files or sorted(f for f in os.listdir(db) if f.endswith(".s") and os.path.exists(os.path.join(da, f)))
    bad = 0
    print("kernel | " + " ".join(r.replace("_count", "").replace("_fixed_size", "") for r in RES) + " | instructions | schedule list (entries)")
    for f in files:
        ka, kb = kernels(os.path.join(da, f)), kernels(os.path.join(db, f))
        print(f"== {f}: {len(ka)} / {len(kb)} kernels")
        for k in sorted(set(ka) | set(kb)):
            if k not in ka or k not in kb:
                print(f"{k}: only in {'A' if k in ka else 'B'}")
                bad += 1
                continue
            (ra, na, sa), (rb, nb, sb) = ka[k], kb[k]
            same_r, same_s = ra == rb, sa == sb
            bad += (not same_r) + (not same_s)
            res = " ".join(str(ra.get(r)) if ra.get(r) == rb.get(r) else f"{ra.get(r)}->{rb.get(r)}" for r in RES)
            print(f"{k} | {res} | {na} -> {nb} | {'same' if same_s else 'DIFFERENT'} ({len(sa)} / {len(sb)})")
    print(f"{bad} difference(s) in resources or schedule lists")
    return bad


if "--tables" in sys.argv:
    a = sys.argv[sys.argv.index("--tables") + 1:]
    sys.exit(1 if tables(a[0], a[1], a[2:]) else 0)
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
