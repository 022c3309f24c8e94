"""The model flag that lets a kernel drop the impedance's ladder on the solimp power (no GPU):
dx_model_load sets DevModel::solimp_pow2 when every solimp a constraint row can take -- dof
friction loss, joint limit, tendon limit, mixed geom pair -- has MuJoCo's default power 2.
dx_model_layout exports it as the last of the specialization dimensions, so a model with any
other power matches no scene specialization and runs the generic kernel, which keeps the
general-power code."""

import ctypes
import glob
import os

import numpy as np
import pytest

from dexterity_amd import _lib, blob, build
from dexterity_amd.mjcf.compiler import CompiledModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = sorted(glob.glob(os.path.join(ROOT, "assets", "*.npz")))
TABLES = ("dof_solimp", "jnt_solimp", "tendon_solimp", "gpair_solimp")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _flag(lib, arrays) -> int:
    b = blob.pack(arrays)
    m = lib.dx_model_load(b, len(b))
    assert m
    buf = (ctypes.c_int32 * 256)()
    n = lib.dx_model_layout(m, buf, 256)
    lib.dx_model_free(m)
    assert n > len(build.DIMS) and build.DIMS[-1] == "solimp_pow2"
    return int(buf[n - 1])


def test_assets_are_found():
    assert len(ASSETS) >= 5


@pytest.mark.parametrize("path", ASSETS, ids=[os.path.basename(p) for p in ASSETS])
def test_shipped_asset_is_all_power_2(lib, path):
    assert _flag(lib, CompiledModel.load(path).arrays) == 1


@pytest.mark.parametrize("path", ASSETS, ids=[os.path.basename(p) for p in ASSETS])
def test_one_changed_power_clears_the_flag(lib, path):
    """A copy with a single entry's power changed, in each table the scene has rows in: the
    first entry and the last one."""
    cm = CompiledModel.load(path)
    tried = 0
    for tab in TABLES:
        a = np.asarray(cm.arrays[tab]).reshape(-1, 5)
        for row in sorted({0, a.shape[0] - 1} if a.shape[0] else ()):
            for power in (1.0, 3.0):
                arrays = {k: np.array(v, copy=True) for k, v in cm.arrays.items()}
                t = arrays[tab].reshape(-1, 5)
                t[row, 4] = power
                arrays[tab] = t.reshape(cm.arrays[tab].shape)
                assert _flag(lib, arrays) == 0, (tab, row, power)
                tried += 1
    assert tried >= 4


def test_specializations_carry_the_constant():
    """Every shipped scene's specialization is a power-2 kernel."""
    text = open(os.path.join(ROOT, "dexterity_amd", "csrc", "dx_specs.inc")).read()
    assert text.count("struct DxSpec_") == text.count("solimp_pow2 = 1") > 0
