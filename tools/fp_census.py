"""Per-source-line census of the fp32 arithmetic of a kernel in a gfx950 assembly listing.

Under -ffp-contract=fast a change of control flow (a loop that becomes straight-line code,
two basic blocks that merge) can make the compiler fuse, or stop fusing, a multiply-add
pair far away from the edit, and the last bit of a result moves.  This tool finds such
pairs without a GPU: it attributes every fp32 / packed-fp32 multiply-add, multiply and
add / subtract of a kernel to the source line of the `.loc` before it and compares two
listings line by line.

  python tools/fp_census.py LISTING.s [KERNEL]            per-line (fused, mul, add) and totals
  python tools/fp_census.py --diff A.s B.s [KERNEL]       the lines whose triples differ
         [--map FILE:DELTA@LINE ...]                      B's FILE has DELTA more lines from LINE on
         [--map-from CSRC_A CSRC_B]                       ... the map from a diff of the sources
  python tools/fp_census.py --compile DIR [--rev=REV] [UNIT ...]   listings of the dx_step.hip units
  python tools/fp_census.py --diff-dirs DIR_A DIR_B       --diff over every unit of two such DIRs
  python tools/fp_census.py --check-line-tables DIR       -gline-tables-only changes no instruction

KERNEL is a substring of the kernel's symbol; without it every kernel of the listing is
counted (matched by symbol in a diff).  A line whose triple only scaled by a common factor
is marked `copies`: an inlined copy of the line appeared or vanished, no fusion changed.

Reading a diff.  One fusion that appears moves the kernel's totals by (+1, -1, -1), one
that vanishes by (-1, +1, +1); a copy that appears or vanishes moves them by its own mix.
The scheduler interleaves neighbouring statements, so single instructions also change the
line they are attributed to (a multiply moves from line 565 to 569 and both lines are
flagged): when the kernel's multiply and add totals are the parent's, the flagged lines are
such moves.  A matching census is necessary, not sufficient (the same counts can hide
another pairing inside a*b + c*d): the bit-exact goldens decide."""
import collections
import concurrent.futures
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from asm_counts import kernel_lines  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_ENC = r"(?:_e32|_e64|_dpp|_sdwa|_e64_dpp)?$"
_FUSED = re.compile(r"^v_(?:pk_)?(?:fma|fmac|mac|mad|fmaak|fmamk|madak|madmk)(?:_legacy)?_f32" + _ENC)
_MUL = re.compile(r"^v_(?:pk_)?mul(?:_legacy)?_f32" + _ENC)
_ADD = re.compile(r"^v_(?:pk_)?(?:add|sub|subrev)_f32" + _ENC)
_FILE = re.compile(r'^\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?')
_LOC = re.compile(r"^\.loc\s+(\d+)\s+(\d+)")


def fp_class(op: str):
    """0 fused multiply-add, 1 multiply, 2 add / subtract, None anything else."""
    for k, rx in enumerate((_FUSED, _MUL, _ADD)):
        if rx.match(op):
            return k
    return None


def file_table(path: str) -> dict:
    """.file number -> base name (the directives stand anywhere in the listing)."""
    table = {}
    for line in open(path, errors="replace"):
        m = _FILE.match(line.strip())
        if m:
            table[int(m.group(1))] = os.path.basename(m.group(3) or m.group(2))
    return table


def kernel_names(path: str) -> list:
    return re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(path, errors="replace").read(), re.M)


def parse_map(items) -> list:
    """['dx_device.h:+3@120', ...] -> [(file, delta, line)]"""
    out = []
    for it in items:
        m = re.match(r"^(.+):([+-]?\d+)@(\d+)$", it)
        if not m:
            raise ValueError(f"line map entry {it!r} is not FILE:DELTA@LINE")
        out.append((m.group(1), int(m.group(2)), int(m.group(3))))
    return out


def map_from_sources(dir_a: str, dir_b: str) -> list:
    """The line map of every source file that both directories hold, from a diff of the
    two versions: where dir_b's file gained (lost) lines against dir_a's."""
    import difflib

    out = []
    for f in sorted(set(os.listdir(dir_a)) & set(os.listdir(dir_b))):
        if not f.endswith((".h", ".hip", ".inc")):
            continue
        a, b = (open(os.path.join(d, f), errors="replace").read().split("\n") for d in (dir_a, dir_b))
        for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
            if tag != "equal" and (j2 - j1) != (i2 - i1):
                out.append((f, (j2 - j1) - (i2 - i1), j2 + 1))
    return out


def census(path: str, name: str, line_map=()) -> dict:
    """{(file, line): [fused, mul, add]} of the first kernel whose symbol contains name.
    line_map entries (file, delta, line) state that this listing's file has delta more
    lines from line on than the listing it is compared with: such lines are renumbered."""
    files = file_table(path)
    out = collections.defaultdict(lambda: [0, 0, 0])
    where = ("?", 0)
    for s in kernel_lines(path, name):
        if not s or s.startswith((";", "//")) or s.endswith(":"):
            continue
        if s.startswith("."):
            m = _LOC.match(s)
            if m:
                f, n = files.get(int(m.group(1)), f"file{m.group(1)}"), int(m.group(2))
                n -= sum(d for mf, d, ml in line_map if mf == f and n >= ml)
                where = (f, n)
            continue
        k = fp_class(s.split()[0])
        if k is not None:
            out[where][k] += 1
    return dict(out)


def totals(c: dict) -> tuple:
    return tuple(sum(v[k] for v in c.values()) for k in range(3))


def scaled(a, b) -> bool:
    """b is a with every count multiplied by one common positive factor other than 1."""
    if tuple(a) == tuple(b) or not any(a) or not any(b):
        return False
    return all(a[i] * b[j] == a[j] * b[i] for i in range(3) for j in range(3))


def diff(ca: dict, cb: dict) -> list:
    """[(file, line, triple_a, triple_b, mark)] of the lines whose triples differ; mark is
    'copies' (common factor), 'only-a' / 'only-b' (the line carries fp32 arithmetic in one
    listing only) or 'FUSION' (the mix changed)."""
    rows = []
    for key in sorted(set(ca) | set(cb)):
        a, b = tuple(ca.get(key, (0, 0, 0))), tuple(cb.get(key, (0, 0, 0)))
        if a == b:
            continue
        mark = "copies" if scaled(a, b) else "only-a" if not any(b) else "only-b" if not any(a) else "FUSION"
        rows.append((key[0], key[1], a, b, mark))
    return rows


def format_census(c: dict) -> str:
    lines = [f"{f}:{n}  fused {v[0]} mul {v[1]} add {v[2]}" for (f, n), v in sorted(c.items())]
    t = totals(c)
    lines.append(f"total  fused {t[0]} mul {t[1]} add {t[2]}  ({len(c)} lines)")
    return "\n".join(lines)


def format_diff(rows: list, ta=None, tb=None) -> str:
    lines = [f"{f}:{n}  {a[0]}/{a[1]}/{a[2]} -> {b[0]}/{b[1]}/{b[2]}  {mark}" for f, n, a, b, mark in rows]
    real = sum(1 for r in rows if r[4] != "copies")
    lines.append(f"{len(rows)} lines differ, {real} other than copy-count changes")
    if ta is not None:
        lines.append(f"totals fused/mul/add  {ta[0]}/{ta[1]}/{ta[2]} -> {tb[0]}/{tb[1]}/{tb[2]}")
    return "\n".join(lines)


def diff_listings(pa: str, pb: str, name: str = None, line_map=()) -> str:
    names = [name] if name else [k for k in kernel_names(pa) if k in set(kernel_names(pb))]
    out = []
    for k in names:
        ca, cb = census(pa, k), census(pb, k, line_map)
        out.append(f"kernel {k}")
        out.append(format_diff(diff(ca, cb), totals(ca), totals(cb)))
    return "\n".join(out)


# ----------------------------------------------------------------------------------------- #
# the driver: listings of every unit build.py compiles from dx_step.hip
# ----------------------------------------------------------------------------------------- #
def step_units() -> list:
    from dexterity_amd import build as B

    return [(n, extra) for n, src, extra in B._units() if src == "dx_step.hip"]


def _checkout(rev: str, dst: str) -> str:
    os.makedirs(dst, exist_ok=True)
    files = subprocess.run(["git", "-C", ROOT, "ls-tree", "--name-only", f"{rev}:dexterity_amd/csrc"],
                           check=True, capture_output=True, text=True).stdout.split()
    for f in files:
        data = subprocess.run(["git", "-C", ROOT, "show", f"{rev}:dexterity_amd/csrc/{f}"], check=True,
                              capture_output=True).stdout
        open(os.path.join(dst, f), "wb").write(data)
    return dst


def compile_units(outdir: str, rev: str = None, units=None, line_tables: bool = True, extra=(), jobs: int = 8) -> list:
    """DIR/<unit>.s for every dx_step.hip unit (or those named), with build.py's FLAGS plus
    -gline-tables-only -S --cuda-device-only; the sources of a git revision with rev."""
    sys.path.insert(0, ROOT)
    from dexterity_amd import build as B

    os.makedirs(outdir, exist_ok=True)
    csrc = _checkout(rev, os.path.join(outdir, "csrc")) if rev else B.CSRC
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmds = []
    for n, uextra in step_units():
        if units and n not in units:
            continue
        out = os.path.join(outdir, f"{n}.s")
        cmds.append(([hipcc, *B.FLAGS, *uextra, *extra, *(("-gline-tables-only",) if line_tables else ()), "-S",
                      "--cuda-device-only", os.path.join(csrc, "dx_step.hip"), "-o", out], out))
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, jobs)) as ex:
        for f in [ex.submit(subprocess.run, c, check=True) for c, _ in cmds]:
            f.result()
    return [o for _, o in cmds]


def instruction_stream(path: str) -> list:
    """The listing's instructions and labels, without directives, comments and blank lines."""
    out = []
    for line in open(path, errors="replace"):
        s = line.split(";")[0].split("//")[0].strip()
        if not s or (s.startswith(".") and not re.match(r"^\.LBB\w+:", s)):
            continue  # (a basic block's label is part of the stream; .Ltmp serve the line tables)
        if s.startswith("__hip_cuid_"):
            continue  # (the compilation unit's id symbol: a hash of the command line)
        out.append(" ".join(s.split()))
    return out


def check_line_tables(outdir: str, unit: str = "dx_step_DxSpec_shadow_reorient") -> str:
    a = compile_units(os.path.join(outdir, "with_tables"), units=[unit])[0]
    b = compile_units(os.path.join(outdir, "without_tables"), units=[unit], line_tables=False)[0]
    sa, sb = instruction_stream(a), instruction_stream(b)
    same = sa == sb
    return (f"{unit}: {len(sa)} instructions and labels with -gline-tables-only, {len(sb)} without: "
            f"{'identical streams' if same else 'STREAMS DIFFER'}")


def diff_dirs(da: str, db: str, line_map=()) -> str:
    out = []
    for n, _ in step_units():
        pa, pb = os.path.join(da, f"{n}.s"), os.path.join(db, f"{n}.s")
        if os.path.exists(pa) and os.path.exists(pb):
            out.append(f"== unit {n}")
            out.append(diff_listings(pa, pb, None, line_map))
    return "\n".join(out)


def main(argv):
    args = list(argv)
    line_map = []
    while "--map" in args:
        i = args.index("--map")
        line_map.append(args[i + 1])
        del args[i:i + 2]
    line_map = parse_map(line_map)
    if "--map-from" in args:  # the map from the two source directories themselves
        i = args.index("--map-from")
        line_map += map_from_sources(args[i + 1], args[i + 2])
        del args[i:i + 3]
    rev = next((a[len("--rev="):] for a in args if a.startswith("--rev=")), None)
    args = [a for a in args if not a.startswith("--rev=")]
    sys.path.insert(0, ROOT)
    if args and args[0] == "--diff":
        print(diff_listings(args[1], args[2], args[3] if len(args) > 3 else None, line_map))
    elif args and args[0] == "--compile":
        for o in compile_units(args[1], rev=rev, units=args[2:] or None):
            print(o)
    elif args and args[0] == "--diff-dirs":
        print(diff_dirs(args[1], args[2], line_map))
    elif args and args[0] == "--check-line-tables":
        print(check_line_tables(args[1]))
    elif args:
        for k in ([args[1]] if len(args) > 1 else kernel_names(args[0])):
            print(f"kernel {k}")
            print(format_census(census(args[0], k)))
    else:
        print(__doc__)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
