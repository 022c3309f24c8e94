"""build.py's unit list and build key (no GPU): every dx_step.hip unit has an instrumented
twin compiled with the profiler flag, the key the library carries covers every unit's own
flags, and a library without a key is refused with a DxError."""

import ctypes
import os
import subprocess

import pytest

from dexterity_amd import _lib, build


def test_every_step_unit_has_a_twin():
    units = build._units()
    names = [n for n, _, _ in units]
    assert len(names) == len(set(names))
    step = {n: extra for n, src, extra in units if src == "dx_step.hip"}
    prod = {n: extra for n, extra in step.items() if build.PROF_FLAG not in extra}
    # the generic unit, one per specialization, the two tiers
    assert set(prod) == {"dx_step", "dx_step_hi", "dx_step_mid"} | {f"dx_step_{s}" for s in build._spec_names()}
    assert len(build._spec_names()) >= 5
    for n, extra in prod.items():
        assert step.get(n + "_prof") == extra + (build.PROF_FLAG,), n
    assert len(step) == 2 * len(prod)
    # no other unit is built with the profiler
    assert all(build.PROF_FLAG not in extra for n, src, extra in units if src != "dx_step.hip")


def test_source_key_covers_the_units_flags(monkeypatch):
    for k in ("DX_PGS_WAVES", "DX_CG_WAVES", "DX_REACH_WAVES"):
        monkeypatch.delenv(k, raising=False)
    base = build.source_key()
    assert base == build.source_key()
    monkeypatch.setenv("DX_PGS_WAVES", "2")  # a specialization's wave count
    waves = build.source_key()
    assert waves != base
    monkeypatch.delenv("DX_PGS_WAVES")
    monkeypatch.setattr(build, "PROF_FLAG", "-DDX_PROF=2")  # the profiler flag
    prof = build.source_key()
    assert prof not in (base, waves)
    monkeypatch.undo()
    assert build.source_key() == base


def test_library_without_a_key_is_refused(tmp_path, monkeypatch):
    src = tmp_path / "nokey.c"
    src.write_text("int dx_abi_version(void) { return 1; }\n")
    lib = tmp_path / "libnokey.so"
    cc = next((c for c in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang") if
               subprocess.run(["sh", "-c", f"command -v {c}"], capture_output=True).returncode == 0), None)
    assert cc, "no C compiler (the oracle needs one too)"
    subprocess.run([cc, "-shared", "-fPIC", str(src), "-o", str(lib)], check=True)
    assert not hasattr(ctypes.CDLL(str(lib)), "dx_build_key")
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.DxError, match="dx_build_key"):
        _lib.load(str(lib))
    assert _lib._lib is None and os.path.exists(lib)
