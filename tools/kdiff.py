"""Device-code diff against an earlier commit: python tools/kdiff.py REV [FILE.hip ...]  -> for every source of build.SOURCES (or the named ones) the
gfx950 assembly of REV's copy and of the working tree's (the product flags + --cuda-device-only -S), compared per kernel: the instruction stream
(comments and directives stripped, the function index taken out of .LBBn_ labels) and VGPRs / AGPRs / SGPRs / LDS / scratch / kernel-argument bytes.
Prints one line per source, every kernel that differs or exists on one side only, and exits 1 if a kernel present on both sides differs.
--table also prints one line per kernel; --keep DIR leaves the .s files there."""
import difflib, hashlib, importlib, os, re, shutil, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import cgs_amd
b = importlib.import_module(cgs_amd.__name__ + ".build")

args = sys.argv[1:]
table = "--table" in args
if table:
    args.remove("--table")
keep = None
if "--keep" in args:
    i = args.index("--keep")
    keep = args[i + 1]
    del args[i:i + 2]
rev, only = args[0], args[1:]
tmp = keep or tempfile.mkdtemp(prefix="cgs_kdiff_")
pkg = os.path.basename(b.HERE)
for d in ("old/csrc", "old/include", "old/s", "new/s"):
    os.makedirs(f"{tmp}/{d}", exist_ok=True)
for f in subprocess.check_output(["git", "ls-tree", "-r", "--name-only", rev, f"{pkg}/csrc/", "include/"], cwd=b.REPO, text=True).split():
    dst = tmp + ("/old/include/" if f.startswith("include/") else "/old/csrc/") + os.path.basename(f)
    with open(dst, "wb") as fp:
        fp.write(subprocess.check_output(["git", "show", f"{rev}:{f}"], cwd=b.REPO))
sides = {"old": (f"{tmp}/old/csrc", f"{tmp}/old/include"), "new": (b.CSRC, os.path.join(b.REPO, "include"))}
srcs = only or b.SOURCES


def compile_one(job):
    side, src = job
    csrc, inc = sides[side]
    out = f"{tmp}/{side}/s/{src.replace('.hip', '.s')}"
    if not os.path.exists(f"{csrc}/{src}"):
        return
    if side == "old" and keep and os.path.exists(out):
        return
    cmd = [b._hipcc(), "-O3", f"--offload-arch={b.ARCH}", "-std=c++17", "-I", inc, "-I", csrc] + b.EXTRA_FLAGS.get(src, []) + ["--cuda-device-only", "-S", f"{csrc}/{src}", "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(f"{side} {src}:\n{r.stderr}")


with ThreadPoolExecutor(max_workers=int(os.environ.get("KDIFF_JOBS", "8"))) as ex:
    list(ex.map(compile_one, [(s, f) for s in ("old", "new") for f in srcs]))

KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size")


def kernels(path):
    """{kernel: (resources tuple, instruction lines)}"""
    if not os.path.exists(path):
        return {}
    txt = open(path).read()
    res = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:", txt, re.S):
        blk = m.group(0)
        g = lambda k: re.search(r"\.%s:\s+(\S+)" % k, blk).group(1)
        res[g("name")] = tuple(int(g(k)) for k in KEYS)
    out, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^([A-Za-z_][\w$.]*):", line)
        if m and m.group(1) in res:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";")[0].strip()
        if not s or (s.startswith(".") and not s.endswith(":")):
            continue
        cur.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return {k: (res[k], out.get(k, [])) for k in res}


def demangle(names):
    if not names:
        return {}
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/lib/llvm/bin")
    if not filt:
        return {n: n for n in names}
    r = subprocess.run([filt] + list(names), capture_output=True, text=True)
    d = r.stdout.strip().split("\n") if r.returncode == 0 else list(names)
    return dict(zip(names, d))


bad = 0
tot = [0, 0, 0, 0]
for src in srcs:
    o, n = kernels(f"{tmp}/old/s/{src.replace('.hip', '.s')}"), kernels(f"{tmp}/new/s/{src.replace('.hip', '.s')}")
    dm = demangle(sorted(set(o) | set(n)))
    same = [k for k in o if k in n and o[k] == n[k]]
    diff = [k for k in o if k in n and o[k] != n[k]]
    gone = [k for k in o if k not in n]
    added = [k for k in n if k not in o]
    for i, l in enumerate((same, diff, gone, added)):
        tot[i] += len(l)
    print(f"{src:22s} kernels old {len(o):3d} new {len(n):3d}  identical {len(same):3d}  differ {len(diff)}  removed {len(gone)}  added {len(added)}")
    if table:
        for k in same:
            h = hashlib.sha1("\n".join(n[k][1]).encode()).hexdigest()[:10]
            print(f"    = {dm[k][:90]:90s} insns {len(n[k][1]):5d} sha1 {h}  v/a/s/lds/scr/karg {'/'.join(map(str, n[k][0]))}")
    for k in gone:
        print(f"    - removed: {dm[k]}  ({len(o[k][1])} lines, res {o[k][0]})")
    for k in added:
        print(f"    + added:   {dm[k]}  ({len(n[k][1])} lines, res {n[k][0]})")
    for k in diff:
        bad += 1
        print(f"    ! differs: {dm[k]}\n        res {o[k][0]} -> {n[k][0]}  lines {len(o[k][1])} -> {len(n[k][1])}")
        for i, l in enumerate(difflib.unified_diff(o[k][1], n[k][1], lineterm="", n=1)):
            if i > 60:
                print("        ...")
                break
            print("        " + l)
print(f"total: identical {tot[0]}  differ {tot[1]}  removed {tot[2]}  added {tot[3]}")
sys.exit(1 if bad else 0)
