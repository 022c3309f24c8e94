"""Records tests/golden/model_tables_parent.json: what dx_model_load derives from the
models of tests/test_model_tables_host.py, at a revision that still has dx_api.hip (the
whole host layer in one translation unit, dx_model private to it).  No GPU is needed.

  python tools/build_variant.py --rev=<revision> parent
  python tools/record_model_tables_golden.py <revision> parent

The first command leaves that revision's sources in variants/parent/csrc and its library
in variants/parent/libdx.so.  This tool compiles a copy of that dx_api.hip with
tests/csrc/dx_model_dump.cpp included at its end as a hook (-DDX_DUMP_HOOK: the dump routine
and its main, inside the unit that defines dx_model), links it against that library for
the kernel launchers, and runs it over the same blobs as the test.  Nothing of the copy is
kept.  Record from the parent of a change to the model compiler, never from the changed
code: if the tables differ for a well-formed model, the change is wrong.
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dexterity_amd import build as B  # noqa: E402
from tests import test_model_tables_host as T  # noqa: E402


def main():
    rev, name = sys.argv[1], sys.argv[2]
    vdir = os.path.join(ROOT, "variants", name)
    api = os.path.join(vdir, "csrc", "dx_api.hip")
    if not os.path.exists(api) or not os.path.exists(os.path.join(vdir, "libdx.so")):
        sys.exit(f"{vdir} has no csrc/dx_api.hip and libdx.so: run tools/build_variant.py --rev={rev} {name} first")
    sha = subprocess.run(["git", "-C", ROOT, "rev-parse", rev], check=True, capture_output=True, text=True).stdout.strip()
    committed = subprocess.run(["git", "-C", ROOT, "show", f"{sha}:dexterity_amd/csrc/dx_api.hip"], check=True,
                               capture_output=True).stdout
    if committed != open(api, "rb").read():
        sys.exit(f"{api} is not {rev}'s dx_api.hip")
    # outside csrc (build.py compiles every unit there), at the same depth for "../../include/dx.h"
    os.makedirs(os.path.join(vdir, "hook"), exist_ok=True)
    hooked = os.path.join(vdir, "hook", "dx_api_dump_hook.hip")
    prog = os.path.join(vdir, "dx_model_dump")
    try:
        with open(hooked, "wb") as f:
            f.write(committed + f'\n#define DX_DUMP_HOOK\n#include "{T.MAIN}"\n'.encode())
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *B.FLAGS, "-I", os.path.dirname(api), hooked, "-o", prog, "-L", vdir,
                        "-l:libdx.so", f"-Wl,-rpath,{vdir}", "-L/opt/rocm/lib", "-lrccl"], check=True)
    finally:
        if os.path.exists(hooked):
            os.remove(hooked)
    with tempfile.TemporaryDirectory() as tmp:
        cases = T.dump_cases(prog, tmp)
    os.remove(prog)
    for case, text in T.EXPECTED_ERRORS.items():
        if cases[case] != ["error: " + text]:
            sys.exit(f"refusing to write: {case} gave {cases[case]}")
    golden = {
        "recorded_from": sha,
        "how": f"python tools/build_variant.py --rev={sha[:7]} {name} && "
               f"python tools/record_model_tables_golden.py {sha[:7]} {name}",
        "format": "per case, the lines of tests/csrc/dx_model_dump.cpp: table, dtype, elements, FNV-1a 64 of the bytes",
        "cases": cases,
    }
    head = {k: v for k, v in golden.items() if k != "cases"}
    with open(T.GOLDEN, "w") as f:  # one line per case
        f.write(json.dumps(head, indent=0, sort_keys=True)[:-2] + ',\n"cases": {\n')
        f.write(",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in sorted(cases.items())))
        f.write("\n}\n}\n")
    print(f"wrote {T.GOLDEN} ({os.path.getsize(T.GOLDEN)} bytes, {len(cases)} cases)")


if __name__ == "__main__":
    main()
