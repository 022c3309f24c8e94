"""Cost of the depth / segmentation cameras: reorient at 4096 envs, one
84 x 84 camera (depth + segmentation), the hand posed by 30 random-agent control steps.
Per camera (`front_close`, and the close `near_top` of the tests) and per cull setting:
HIP-event time of each of 100 renders behind 10 warm-up renders, and the geoms that survive
the per-tile cull (mean and maximum per tile).  Beside them the control step's wall-clock ms
with cameras off and on (one synchronisation at the end of the timed steps).  Ahead of them,
per camera, depth only against depth + shaded RGB under the default lights (one shadow-casting
light): ms per control step, ms per render, and the geoms that survive the shadow cull per
tile.  One JSON line per case.

    python tools/camera_cost.py [--envs 4096] [--side 84] [--renders 100] [--steps 200]
"""

import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dexterity_amd import _lib, cameras, manipulation  # noqa: E402

NEAR_TOP = cameras.CameraConfig("near_top", (-0.02, -0.02, 0.55), (1, 0, 0, 0, 1, 0))
CAMERAS = (cameras.FRONT_CLOSE, NEAR_TOP)


def event_times(hip, stream, fn, n):
    """ms of each of n calls of fn, between HIP events on `stream`."""
    vp = ctypes.c_void_p
    hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
    hip.hipEventRecord.argtypes = [vp, vp]
    hip.hipEventSynchronize.argtypes = [vp]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]
    hip.hipEventDestroy.argtypes = [vp]
    pairs = []
    for _ in range(n):
        a, b = vp(), vp()
        assert hip.hipEventCreate(ctypes.byref(a)) == 0 and hip.hipEventCreate(ctypes.byref(b)) == 0
        assert hip.hipEventRecord(a, stream) == 0
        fn()
        assert hip.hipEventRecord(b, stream) == 0
        pairs.append((a, b))
    out = []
    for a, b in pairs:
        assert hip.hipEventSynchronize(b) == 0
        ms = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(ms), a, b) == 0
        out.append(ms.value)
        hip.hipEventDestroy(a)
        hip.hipEventDestroy(b)
    return out


def step_ms(env, k0, steps):
    env.physics.sync()
    t0 = time.perf_counter()
    for k in range(k0, k0 + steps):
        env.step_random(k)
    env.physics.sync()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--side", type=int, default=84)
    ap.add_argument("--renders", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rgb-only", action="store_true", help="only the depth against depth + RGB rows")
    a = ap.parse_args()
    L = _lib.load()
    hip = manipulation._hip_runtime()
    env = manipulation.load("reorient", "state_dense", seed=1, num_envs=a.envs)
    env.reset()
    for k in range(a.warmup):
        env.step_random(k)
    k = a.warmup
    off_ms = step_ms(env, k, a.steps)
    k += a.steps
    print(json.dumps({"config": f"3 reorient {a.envs}, cameras off", "ms_per_step": round(off_ms, 4)}), flush=True)
    stream = ctypes.c_void_p(L.dx_stream(env.physics.ptr))
    tiles = ((a.side + 15) // 16) ** 2
    # depth only against depth + RGB under the default lights (one shadow-casting light)
    for cam in CAMERAS:
        row = {"config": f"3 reorient {a.envs}, {cam.name} {a.side}x{a.side}: depth only / depth + RGB"}
        for rgb in (False, True):
            env.enable_cameras([cam], height=a.side, width=a.side, depth=True, segmentation=False, rgb=rgb)
            row["ms_per_step_depth_rgb" if rgb else "ms_per_step_depth"] = round(step_ms(env, k, a.steps), 4)
            k += a.steps
            env.physics.set_cameras([cam], a.side, a.side, depth=True, segmentation=False, rgb=rgb)
            for _ in range(10):
                env.physics.render()
            ms = event_times(hip, stream, env.physics.render, a.renders)
            row["render_ms_mean_depth_rgb" if rgb else "render_ms_mean_depth"] = round(sum(ms) / len(ms), 4)
        env.physics.render_stats(True)
        env.physics.shadow_stats()
        env.physics.render()
        env.physics.render_stats(False)
        total, most, passes = env.physics.shadow_stats()
        row.update(ms_per_step_cameras_off=round(off_ms, 4), shadow_survivors_per_tile_mean=round(total / max(passes, 1), 2),
                   shadow_survivors_per_tile_max=most, shadow_passes=passes, tiles=a.envs * tiles)
        print(json.dumps(row), flush=True)
        env.enable_cameras([])
    for cam in () if a.rgb_only else CAMERAS:
        env.enable_cameras([cam], height=a.side, width=a.side, depth=True, segmentation=True)
        on_ms = step_ms(env, k, a.steps)
        k += a.steps
        images = {}
        for cull in (True, False):
            # the env's batch, the cameras set at the batch level (body poses stay on)
            env.physics.set_cameras([cam], a.side, a.side, depth=True, segmentation=True, cull=cull)
            for _ in range(10):
                env.physics.render()
            ms = event_times(hip, stream, env.physics.render, a.renders)
            env.physics.render_stats(True)
            env.physics.render()
            total, most, ntile = env.physics.render_stats(False)
            images[cull] = (env.physics.depth(), env.physics.segmentation())
            print(json.dumps({
                "config": f"3 reorient {a.envs}, {cam.name} {a.side}x{a.side}, cull {'on' if cull else 'off'}",
                "rays": a.envs * a.side * a.side, "renders": len(ms),
                "render_ms_mean": round(sum(ms) / len(ms), 4), "render_ms_min": round(min(ms), 4),
                "render_ms_max": round(max(ms), 4),
                "survivors_per_tile_mean": round(total / max(ntile, 1), 2), "survivors_per_tile_max": most,
                "tiles": ntile, "tiles_per_image": tiles, "geoms": env.model.ngeom,
                "hit_share": round(float((images[cull][1] >= 0).mean()), 4),
                "object_share": round(float((images[cull][1] > 0).mean()), 4)}), flush=True)
        same = (images[True][0].view("uint32") == images[False][0].view("uint32")).all() and \
            (images[True][1] == images[False][1]).all()
        print(json.dumps({"config": f"3 reorient {a.envs}, {cam.name}: control step with the camera on",
                          "ms_per_step": round(on_ms, 4), "ms_per_step_cameras_off": round(off_ms, 4),
                          "cull_images_bit_identical": bool(same)}), flush=True)
        env.enable_cameras([])
    off2 = step_ms(env, k, a.steps)
    print(json.dumps({"config": f"3 reorient {a.envs}, cameras off again", "ms_per_step": round(off2, 4)}), flush=True)
    env.close()


if __name__ == "__main__":
    main()
