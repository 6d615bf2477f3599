"""Compare the gfx950 device code of two checkouts, kernel by kernel:

    python tools/isa_diff.py TREE_A TREE_B kernels_pt.hip kernels_predict.hip ...

Each named csrc/*.hip of each tree is compiled with the build's flags (build_native.CFLAGS of the
tree itself) plus -S --cuda-device-only, at most 8 compiles at a time.  Comments are stripped, the
function index of basic-block labels (.LBB<n>_) is dropped, and every kernel is cut from its label
to its last s_endpgm.  One line per kernel symbol: lines in A, lines in B, identical or not, and
vgpr_count / spill counts from the code-object metadata.  Exit status 1 if a symbol present in
both trees differs.  The comparison is of text only; no GPU is needed.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import importlib.util
import re
import subprocess
import sys
import tempfile
from pathlib import Path

PKG = "mlff-preconditioner_amd"


def tree_flags(tree: Path):
    """(hipcc, CFLAGS) of the tree's own build_native.py."""
    spec = importlib.util.spec_from_file_location(f"build_native_{abs(hash(tree))}", tree / PKG / "build_native.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.HIPCC, list(mod.CFLAGS)


def compile_asm(tree: Path, name: str, out: Path) -> str:
    hipcc, cflags = tree_flags(tree)
    cmd = [hipcc, *cflags, "-S", "--cuda-device-only", str(tree / PKG / "csrc" / name), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed for {tree / PKG / 'csrc' / name}:\n{res.stdout}\n{res.stderr}")
    return out.read_text()


_LBB = re.compile(r"\.LBB\d+_")


def kernel_bodies(asm: str) -> dict[str, list[str]]:
    """symbol -> normalised lines from the kernel's label to its last s_endpgm."""
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M))
    bodies: dict[str, list[str]] = {}
    cur, buf = None, []

    def close():
        if cur is None:
            return
        last = max((i for i, ln in enumerate(buf) if ln.startswith("s_endpgm")), default=-1)
        bodies[cur] = buf[: last + 1]

    for raw in asm.splitlines():
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        m = re.fullmatch(r"([A-Za-z_$.][\w$.]*):", line)
        if m and not line.startswith(".L") and m.group(1) in kernels:
            close()
            cur, buf = m.group(1), []
            continue
        if m and not line.startswith(".L") or line.startswith((".section", ".text", ".rodata")):
            close()  # another function's label or a section change ends the kernel
            cur, buf = None, []
            continue
        if cur is not None:
            buf.append(_LBB.sub(".LBB_", line))
    close()
    return bodies


def kernel_meta(asm: str) -> dict[str, dict[str, int]]:
    """symbol -> {vgpr_count, sgpr_spill_count, vgpr_spill_count} from the amdhsa metadata."""
    meta: dict[str, dict[str, int]] = {}
    m = re.search(r"^amdhsa\.kernels:(.*?)^amdhsa\.", asm, flags=re.M | re.S)
    if not m:
        return meta
    for entry in re.split(r"^  - ", m.group(1), flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", entry, flags=re.M)
        if not name:
            continue
        vals = {}
        for key in (".vgpr_count", ".sgpr_spill_count", ".vgpr_spill_count"):
            v = re.search(rf"^\s*{re.escape(key)}:\s*(\d+)", entry, flags=re.M)
            vals[key[1:]] = int(v.group(1)) if v else -1
        meta[name.group(1)] = vals
    return meta


def demangler():
    for p in (Path("/opt/rocm/llvm/bin/llvm-cxxfilt"), Path("/opt/rocm/bin/llvm-cxxfilt")):
        if p.exists():
            return str(p)
    return None


def demangle(names: list[str]) -> dict[str, str]:
    tool = demangler()
    if tool is None or not names:
        return {n: n for n in names}
    res = subprocess.run([tool, *names], capture_output=True, text=True)
    out = res.stdout.splitlines()
    if res.returncode != 0 or len(out) != len(names):
        return {n: n for n in names}
    # drop the argument list and the anonymous namespace: the template arguments tell kernels apart
    short = [re.sub(r"\(anonymous namespace\)::", "", re.sub(r"^void ", "", o)) for o in out]
    short = [re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", s) for s in short]
    return dict(zip(names, short))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a", type=Path)
    ap.add_argument("tree_b", type=Path)
    ap.add_argument("files", nargs="+", help="names of csrc/*.hip files")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    jobs = max(1, min(8, a.jobs))
    with tempfile.TemporaryDirectory() as tmp:
        work = [(side, tree, name, Path(tmp) / f"{side}_{Path(name).stem}.s")
                for name in a.files for side, tree in (("a", a.tree_a), ("b", a.tree_b))]
        with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
            texts = list(ex.map(lambda w: compile_asm(w[1].resolve(), w[2], w[3]), work))
    asm = {(w[0], w[2]): t for w, t in zip(work, texts)}
    differ = 0
    for name in a.files:
        ta, tb = asm[("a", name)], asm[("b", name)]
        ba, bb = kernel_bodies(ta), kernel_bodies(tb)
        ma, mb = kernel_meta(ta), kernel_meta(tb)
        syms = sorted(set(ba) | set(bb))
        pretty = demangle(syms)
        same = sum(1 for s in syms if s in ba and s in bb and ba[s] == bb[s])
        both = sum(1 for s in syms if s in ba and s in bb)
        print(f"{name}: {len(ta.splitlines())} -> {len(tb.splitlines())} assembly lines, "
              f"{same} of {both} common kernels identical")
        for s in syms:
            def side(b, m):
                if s not in b:
                    return "     -  (absent)"
                v = m.get(s, {})
                return (f"{len(b[s]):6d}  vgpr {v.get('vgpr_count', -1):3d} "
                        f"spill s{v.get('sgpr_spill_count', -1)} v{v.get('vgpr_spill_count', -1)}")
            if s in ba and s in bb:
                verdict = "identical" if ba[s] == bb[s] else "DIFFERS"
                differ += ba[s] != bb[s]
            else:
                verdict = "only in A" if s in ba else "only in B"
            print(f"  {verdict:9s}  A {side(ba, ma)}   B {side(bb, mb)}   {pretty[s]}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
