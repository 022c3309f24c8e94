"""numpy replay of the random pushes (include/dx.h dx_env_set_perturbation).

Env e owns RandomState(seed + env0 + e).  Per control step and configured body, in order,
seven random_sample doubles -- u_gate, u_fmag, u_fz, u_fphi, u_tmag, u_tz, u_tphi -- are
consumed whatever happens next, then the first rule that matches applies:
  the step re-initialises the env (it returns FIRST):  remain = 0, wrench = 0;
  remain > 0:                                          remain -= 1, the wrench stays;
  else: wrench = 0, and if u_gate < probability a new push of `duration` control steps.
All in fp64 without fused multiply-adds, each component rounded to fp32 once."""

import numpy as np

FIRST, MID, LAST = 0, 1, 2
DRAWS = 7  # per configured body and control step
# The settings the CPU and the GPU tests share: 16 envs x 30 steps, episodes of 12 control
# steps.  The cube weighs 0.63 N: pushes of a sixth of its weight up to its weight.
SETTINGS = dict(probability=0.25, force_range=(0.1, 0.6), torque_range=(0.0, 0.002), duration=3, seed=11)
NENV, NSTEPS, EPISODE = 16, 30, 12


def direction(u_z, u_phi):
    """Uniform on the sphere: (s cos phi, s sin phi, z), z = 2 u_z - 1, phi = 2 pi u_phi."""
    z = 2.0 * u_z - 1.0
    s = np.sqrt(1.0 - z * z)
    phi = 6.283185307179586 * u_phi
    return np.array([s * np.cos(phi), s * np.sin(phi), z])


def wrench(u, force_range, torque_range):
    """The fp32 (force, torque) of a new push from the step's seven doubles u (u[0] is the gate)."""
    fmag = force_range[0] + (force_range[1] - force_range[0]) * u[1]
    tmag = torque_range[0] + (torque_range[1] - torque_range[0]) * u[4]
    return np.concatenate([fmag * direction(u[2], u[3]), tmag * direction(u[5], u[6])]).astype(np.float32)


class Replay:
    """The pushes of `nenv` envs, one control step at a time; `step(reinit)` takes the mask
    of the envs this step re-initialises (it returns FIRST for them) and returns the
    [nenv, nb, 6] float32 wrenches, DX_OUT_PERTURB's content."""

    def __init__(self, nenv, nb, probability, force_range, torque_range=(0.0, 0.0), duration=1, seed=0, env0=0):
        self.rs = [np.random.RandomState((seed + env0 + e) & 0xFFFFFFFF) for e in range(nenv)]
        self.nenv, self.nb = nenv, nb
        self.probability, self.force_range, self.torque_range, self.duration = (probability, force_range,
                                                                                torque_range, duration)
        self.reset()

    def reset(self):
        """dx_env_reset: no wrench held, nothing drawn."""
        self.remain = np.zeros((self.nenv, self.nb), np.int32)
        self.wrench = np.zeros((self.nenv, self.nb, 6), np.float32)
        self.started = np.zeros((self.nenv, self.nb), bool)

    def step(self, reinit):
        self.started[:] = False
        for e in range(self.nenv):
            u = self.rs[e].random_sample(DRAWS * self.nb).reshape(self.nb, DRAWS)
            for k in range(self.nb):
                if reinit[e]:
                    self.remain[e, k] = 0
                    self.wrench[e, k] = 0
                elif self.remain[e, k] > 0:
                    self.remain[e, k] -= 1
                else:
                    self.wrench[e, k] = 0
                    if u[k, 0] < self.probability:
                        self.remain[e, k] = self.duration - 1
                        self.wrench[e, k] = wrench(u[k], self.force_range, self.torque_range)
                        self.started[e, k] = True
        return self.wrench.copy()


def fixed_episodes(nenv, nsteps, episode):
    """Step types of envs that all run episodes of `episode` control steps after a reset:
    step i (0-based) returns LAST when (i + 1) % (episode + 1) == episode, FIRST on the
    step after a LAST, else MID.  [nsteps, nenv] -- the schedule of a time-limited env, used
    where no device run is at hand."""
    t = np.empty((nsteps, nenv), np.int32)
    for i in range(nsteps):
        r = (i + 1) % (episode + 1)
        t[i] = FIRST if r == 0 else LAST if r == episode else MID
    return t


def replay(step_types, nb, **kw):
    """[nsteps, nenv, nb, 6] wrenches and [nsteps, nenv, nb] push starts for the step types
    [nsteps, nenv] that the steps RETURN after a reset: step i re-initialises an env when
    its step i - 1 returned LAST."""
    nsteps, nenv = step_types.shape
    r = Replay(nenv, nb, **kw)
    out = np.zeros((nsteps, nenv, nb, 6), np.float32)
    started = np.zeros((nsteps, nenv, nb), bool)
    prev = np.full(nenv, FIRST)
    for i in range(nsteps):
        out[i] = r.step(prev == LAST)
        started[i] = r.started
        prev = step_types[i]
    return out, started


def summary(wrenches, started, step_types, duration):
    """What a schedule shows: pushes cut short by an episode reset, pushes that end and are
    followed by a new one on the very next step, and the fraction of non-FIRST env-steps
    that carry a wrench."""
    nsteps, nenv, nb, _ = wrenches.shape
    on = np.abs(wrenches).sum(axis=3) > 0
    cut = back_to_back = 0
    for e in range(nenv):
        for k in range(nb):
            for i in np.nonzero(started[:, e, k])[0]:
                length = 1
                while i + length < nsteps and on[i + length, e, k] and not started[i + length, e, k]:
                    length += 1
                if i + length < nsteps:
                    if length < duration:
                        assert step_types[i + length, e] == FIRST
                        cut += 1
                    else:
                        assert length == duration
                        back_to_back += bool(started[i + length, e, k])
    live = step_types != FIRST
    return dict(cut=cut, back_to_back=back_to_back,
                carrying=float((on.any(axis=2) & live).sum()) / max(1, int(live.sum())))
