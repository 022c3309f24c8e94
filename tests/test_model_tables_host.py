"""The model compiler's tables against the parent revision's, on the host (no GPU).

dexterity_amd/csrc/dx_model.hip is plain host code: tests/csrc/dx_model_dump.cpp links it
alone, with the host compiler and no HIP library, and prints one hash line per table
dx_model_load derives.  The lines are compared with tests/golden/model_tables_parent.json,
recorded by tools/record_model_tables_golden.py from the revision before the host layer was
split (the same dump routine, hooked into that revision's dx_api.hip): the tables the
kernels index must come out bit for bit, and the malformed blobs must be refused with the
same text.  The program is built a second time with -fsanitize=address,undefined and must
print the same lines and exit 0.

A table that dx_batch.hip device_model uploads but the compiler no longer builds fails
here (test_every_uploaded_table_is_dumped), not on the GPU.
"""
import hashlib
import json
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dexterity_amd import blob as blob_mod  # noqa: E402
from dexterity_amd import build as dx_build  # noqa: E402
from dexterity_amd.mjcf.compiler import CompiledModel  # noqa: E402
from tests.conftest import inclined_box_scene, resting_box_scene  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "model_tables_parent.json")
UNIT = os.path.join(dx_build.CSRC, "dx_model.hip")
MAIN = os.path.join(HERE, "csrc", "dx_model_dump.cpp")
OUTDIR = os.path.join(HERE, "_build")
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")
ASSETS = ("adroit_hand", "adroit_reach", "bimanual_handover", "shadow_reach", "shadow_reorient")
DENSE = "shadow_reorient+DX_DENSE_MSOLVE=1"  # the same blob, the switch in the program's environment


def well_formed() -> dict:
    """Case name -> blob: the five assets, the headline scene with the two other solvers,
    and the box scenes (no tendons, no limited joints, a single root: the `empty ? {0}`
    paths)."""
    models = {a: CompiledModel.load(os.path.join(ROOT, "assets", a + ".npz")) for a in ASSETS}
    models["shadow_reorient_cg"] = models["shadow_reorient"].with_solver("CG")
    models["shadow_reorient_pgs"] = models["shadow_reorient"].with_solver("PGS")
    models["inclined_box_10"] = inclined_box_scene(10)
    models["resting_box_1"] = resting_box_scene(1)
    models["resting_box_3"] = resting_box_scene(3)
    return {name: blob_mod.pack(cm.arrays) for name, cm in models.items()}


def malformed() -> dict:
    """Case name -> blob dx_model_load must refuse."""
    arrays = CompiledModel.load(os.path.join(ROOT, "assets", "shadow_reorient.npz")).arrays
    entry = b"x".ljust(48, b"\0") + struct.pack("<iiqq", 1, 0, 4, 80)  # 4 doubles at 80 of an 88-byte file
    return {
        "bad_8_bytes": blob_mod.MAGIC,
        "bad_magic": b"DXMBLOB2" + struct.pack("<q", 0),
        "bad_count_1000": blob_mod.MAGIC + struct.pack("<q", 1000),
        "bad_entry_past_end": blob_mod.MAGIC + struct.pack("<q", 1) + entry,
        "bad_no_gravity": blob_mod.pack({k: v for k, v in arrays.items() if k != "gravity"}),
        "bad_solver_7": blob_mod.pack({**arrays, "solver": np.array([7], np.int32)}),
        "bad_nv_65": blob_mod.pack({**arrays, "nv": np.array([65], np.int32)}),
    }


EXPECTED_ERRORS = {
    "bad_8_bytes": "malformed model blob",
    "bad_magic": "malformed model blob",
    "bad_count_1000": "malformed model blob",
    "bad_entry_past_end": "malformed model blob",
    "bad_no_gravity": "blob missing float array gravity",
    "bad_solver_7": "unknown solver",
    "bad_nv_65": "nv must be in [1, 64]",
}


def build_program(sanitize: bool = False, force: bool = False) -> str:
    """tests/_build/dx_model_dump[_san]: the model unit and the dump program compiled as
    libdx.so's units are (build.py's driver and FLAGS), linked by the host compiler with no
    HIP library.  A program built from the present sources and flags is used as it is."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = os.path.join(OUTDIR, "dx_model_dump_san" if sanitize else "dx_model_dump")
    h = hashlib.sha1(" ".join(dx_build.FLAGS + (SANITIZE if sanitize else ())).encode())
    for path in [UNIT, MAIN, os.path.join(ROOT, "include", "dx.h")] + [os.path.join(dx_build.CSRC, f) for f in dx_build.HEADERS]:
        h.update(open(path, "rb").read())
    key = h.hexdigest()
    if not force and os.path.exists(out) and os.path.exists(out + ".key") and open(out + ".key").read() == key:
        return out
    os.makedirs(OUTDIR, exist_ok=True)
    tmp = f"{out}.{os.getpid()}"
    san = tuple(x for f in SANITIZE for x in ("-Xarch_host", f)) if sanitize else ()  # (the host code only)
    for src, obj in ((UNIT, ".unit.o"), (MAIN, ".main.o")):
        subprocess.run([hipcc, *dx_build.FLAGS, *san, "-c", src, "-o", tmp + obj], check=True)
    cxx = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "clang++")
    subprocess.run([cxx, *(SANITIZE if sanitize else ()), tmp + ".unit.o", tmp + ".main.o", "-o", tmp + ".tmp"], check=True)
    os.replace(tmp + ".tmp", out)
    for part in (".unit.o", ".main.o"):
        os.remove(tmp + part)
    with open(out + ".key", "w") as f:
        f.write(key)
    return out


def run_program(prog: str, blobs: dict, workdir: str, env: dict = None) -> dict:
    """Case name -> the program's lines for that blob.  Must exit 0 with nothing on stderr
    (a sanitizer report goes there)."""
    paths = []
    for name, data in blobs.items():
        paths.append(os.path.join(workdir, name))
        with open(paths[-1], "wb") as f:
            f.write(data)
    base = {k: v for k, v in os.environ.items() if not k.startswith("DX_")}  # (DX_PRINT_LDS writes to stderr)
    r = subprocess.run([prog, *paths], capture_output=True, text=True, env={**base, **(env or {})})
    assert r.returncode == 0 and not r.stderr, f"{prog} exited {r.returncode}:\n{r.stderr[-4000:]}"
    out, cur = {}, None
    for line in r.stdout.splitlines():
        if line.startswith("# "):
            cur = out.setdefault(line[2:], [])
        else:
            cur.append(line)
    assert list(out) == list(blobs)
    return out


def dump_cases(prog: str, workdir: str) -> dict:
    """Every case of the golden through `prog`."""
    good = well_formed()
    out = run_program(prog, {**good, **malformed()}, workdir)
    out[DENSE] = run_program(prog, {"shadow_reorient": good["shadow_reorient"]}, workdir,
                             {"DX_DENSE_MSOLVE": "1"})["shadow_reorient"]
    return out


@pytest.fixture(scope="module")
def golden_tables():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    return dump_cases(build_program(), str(tmp_path_factory.mktemp("model_tables")))


def test_tables_match_parent(dumped, golden_tables):
    cases = golden_tables["cases"]
    assert sorted(dumped) == sorted(cases)
    for name, lines in dumped.items():
        want = cases[name]
        diff = [f"{a!r} != {b!r}" for a, b in zip(lines, want) if a != b]
        assert lines == want, f"{name}: {len(lines)} lines, golden {len(want)}; first differences: {diff[:5]}"


def test_malformed_blobs_are_refused(dumped):
    for name, text in EXPECTED_ERRORS.items():
        assert dumped[name] == ["error: " + text], name


def test_dense_switch_drops_the_ldl_table(dumped):
    """DX_DENSE_MSOLVE=1 is read by the loader: an empty ldl_tab, every other table as without it."""
    a, b = dumped["shadow_reorient"], dumped[DENSE]
    changed = sorted(x.split()[0] for x, y in zip(a, b) if x != y)
    assert len(a) == len(b) and changed == ["dm", "ldl_tab"]
    assert [x for x in b if x.startswith("ldl_tab ")][0].split()[2] == "0"


def test_every_uploaded_table_is_dumped(dumped):
    """dx_batch.hip device_model's upload list (UF / UI) against every well-formed model's dump."""
    src = open(os.path.join(dx_build.CSRC, "dx_batch.hip")).read()
    body = src[src.index("int device_model("):]
    body = body[:body.index("#undef UF")]
    uploaded = [t for t in re.findall(r"\bU[FI]\((\w+)\)", body) if t != "field"]  # (the macros' own parameter)
    assert len(uploaded) > 90 and "body_rec" in uploaded and "ldl_tab" in uploaded
    for name in list(well_formed()) + [DENSE]:
        have = {line.split()[0] for line in dumped[name]}
        assert "body_chain" in have
        missing = [t for t in uploaded if t not in have]
        assert not missing, f"{name}: uploaded but not built: {missing}"


def test_sanitized_build_agrees(dumped, tmp_path):
    """The same program under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone
    executable, nothing preloaded; any report aborts it (-fno-sanitize-recover)."""
    assert dump_cases(build_program(sanitize=True), str(tmp_path)) == dumped
