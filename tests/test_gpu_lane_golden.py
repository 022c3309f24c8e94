"""The lane id's range is scaffolding too: stating it for every LANE of the step kernel
must leave every result as it was.  The bit-exact goldens of test_gpu_guard_golden.py and
test_gpu_broadphase.py hold 16 to 64 envs; tests/golden/lane_parent.npz
(tools/record_lane_golden.py, run with the parent revision's library) widens that to
reorient (Newton) at 256 envs x 12 control steps with the device random agent, as one CRC32
per env of the final qpos | qvel | warm start | observation | reward | discount | step_type
bytes."""

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_lane_golden", os.path.join(ROOT, "tools", "record_lane_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


def test_states_are_the_parents():
    with np.load(os.path.join(ROOT, "tests", "golden", "lane_parent.npz")) as z:
        want, seed = z["crc"], int(z["seed"])
        # the recorded (parent's) run had contacts and an auto-reset in it
        assert float(z["contact_fraction"]) >= REC.BP.MIN_CONTACT_FRACTION and int(z["auto_resets"]) >= 1
    assert want.shape == (REC.NENV,) and want.dtype == np.uint32
    got = REC.run_case(seed)
    h = got["health"]
    assert h["contact_overflow"] == 0 and h["row_overflow"] == 0 and h["diverged"] == 0, h
    differ = np.flatnonzero(got["crc"] != want)
    assert differ.size == 0, f"{differ.size} of {REC.NENV} envs differ from the parent's run, first {differ[:8].tolist()}"
    ok, frac, resets = REC.parent_run_ok(got)
    assert ok, (frac, resets)
