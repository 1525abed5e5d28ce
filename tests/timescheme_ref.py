"""The time scheme (gfv/timescheme.py) restated for the tests.

(a) `LaunchRule`: the rule of `gfv_time_scheme_update` in numpy, written from the paragraph of include/gfv.h - float32 arithmetic,
    one rounding per operation, in the order written there - holding the ring, `ustar`, `dt_eff` and the record.
(b) `stages_ts` / `one_hot_gradients_ts`: the finite-volume section of tests/fvm_float64.py with a separate baseline of the time
    difference: `uv_hat` is formed from `uv_old`, channels 5,6 of phi carry `uv_star` and the time term's step is `dt_eff`.  The
    oracle's integrators already take `uv_hat` and `uv_old` as separate arguments, so nothing of their arithmetic is restated.

Not a conftest, not a test module: imported by name with tests/ on sys.path."""
import numpy as np
import torch

import fvm_float64 as F

f32 = np.float32
BDF1, BDF2 = 1, 2
SCHEME, BASE = 0, 1
THIRD, ONE_AND_A_HALF = f32(3.0), f32(1.5)


# ---- (a) the launch ------------------------------------------------------------------------------------------------------------
class LaunchRule:
    def __init__(self, batch, uvp_dim, dt, scheme=BDF2):
        self.batch = np.asarray(batch, dtype=np.int64)
        self.uvp_dim = np.asarray(uvp_dim, dtype=f32).reshape(-1, 3)
        self.dt = np.asarray(dt, dtype=f32).reshape(-1)
        N, B = self.batch.shape[0], self.dt.shape[0]
        self.ring = np.zeros((2, N, 2), dtype=f32)
        self.ustar = np.zeros((N, 2), dtype=f32)
        self.dt_eff = np.zeros(B, dtype=f32)
        self.rec = np.zeros(4, dtype=np.int32)
        self.rec[SCHEME] = scheme

    # the host's side: what gfv.timescheme.TimeScheme writes in front of a launch
    def reset(self, clock):
        """History forgotten: base = the current clock."""
        self.rec[BASE] = clock

    def install_previous(self, previous, clock):
        """`previous` [N, >= 2] becomes field clock - 1: the slot the launch at `clock` reads; base = clock - 1."""
        self.ring[(clock & 1) ^ 1] = np.asarray(previous, dtype=f32)[:, 0:2]
        self.rec[BASE] = clock - 1

    def active(self, clock):
        return bool(self.rec[SCHEME] == BDF2 and clock > self.rec[BASE])

    def launch(self, x_backup, clock):
        """One launch that finds `clock`: x_backup [N, 12] holds field `clock`."""
        cur = np.asarray(x_backup, dtype=f32)[:, 0:2]
        dim = self.uvp_dim[self.batch][:, 0:2]
        active = self.active(clock)
        slot = clock & 1
        if active:
            prev = self.ring[slot ^ 1]
            d = (cur - prev).astype(f32)
            q = (d / THIRD).astype(f32)
            s = (cur + q).astype(f32)
            self.ustar = (s / dim).astype(f32)
            self.dt_eff = (self.dt / ONE_AND_A_HALF).astype(f32)
        else:
            self.ustar = (cur / dim).astype(f32)
            self.dt_eff = self.dt.copy()
        self.ring[slot] = cur
        return active

    def state(self):
        return dict(ring=self.ring.copy(), ustar=self.ustar.copy(), dt_eff=self.dt_eff.copy())


def ustar_of(cur, prev, batch, uvp_dim):
    """The active launch's baseline from two fields [N, >= 2] (float32 numpy): cur + (cur - prev) / 3, then / uvp_dim."""
    cur, prev = np.asarray(cur, dtype=f32)[:, 0:2], np.asarray(prev, dtype=f32)[:, 0:2]
    dim = np.asarray(uvp_dim, dtype=f32).reshape(-1, 3)[np.asarray(batch, dtype=np.int64)][:, 0:2]
    s = (cur + ((cur - prev).astype(f32) / THIRD).astype(f32)).astype(f32)
    return (s / dim).astype(f32)


# ---- (b) the section with a separate baseline ------------------------------------------------------------------------------------
def with_step(G, dt_eff):
    """A copy of G whose time step is dt_eff [B] (in G's dtype and dt_graph's shape)."""
    dt = torch.as_tensor(dt_eff).to(G["dt_graph"].dtype).reshape(G["dt_graph"].shape)
    return dict(G, dt_graph=dt)


def stages_ts(dec, uv_old, uv_star, dt_eff, G, conserved=True, integrator="imex", order="2nd"):
    """fvm_float64.stages with uv_hat from `uv_old`, the baseline `uv_star` where uv_old goes (phi[:, 5:7], the integrator's
    third argument) and the step `dt_eff`.  fvm_float64.stages forms phi through the module's `phi_stage`, handing it the tensor
    it also hands the integrator: for the duration of the call that name is a function that forms uv_hat from `uv_old` and puts
    what it was handed - the baseline - into channels 5,6."""
    orig = F.phi_stage

    def phi_stage(dec_, y, node_type, baseline, integrator_):
        phi = orig(dec_, y, node_type, uv_old, integrator_)
        return torch.cat((phi[:, 0:5], baseline, phi[:, 7:8]), dim=1)

    F.phi_stage = phi_stage
    try:
        return F.stages(dec, uv_star, with_step(G, dt_eff), conserved, integrator, order)
    finally:
        F.phi_stage = orig


def one_hot_gradients_ts(dec, uv_old, uv_star, dt_eff, G, conserved=True, integrator="imex", order="2nd"):
    """fvm_float64.one_hot_gradients of `stages_ts`."""
    dec = dec.detach().clone().requires_grad_(True)
    losses = stages_ts(dec, uv_old, uv_star, dt_eff, G, conserved, integrator, order)["losses"]
    outflow = F.has_outflow(G)
    grads = {}
    for b in range(G["num_graphs"]):
        for l in range(4):
            if l == 3 and not bool(outflow[b]):
                continue
            grads[(b, l)] = torch.autograd.grad(losses[b, l], dec, retain_graph=True)[0]
    return grads


def draw_baseline(uv_old, dt, seed):
    """A baseline and a step far enough from (uv_old, dt) that a section reading either in the other's place is seen in the
    momentum columns of cres: uv_star = uv_old + 10 randn per node and channel, dt_eff = dt / 4, in float32.  Chosen on the CPU
    (tests/test_timescheme_gpu.py asserts it): on the small polygon mesh the float32 oracle's own cres error is 1.7e-4 - the
    time term is a small part of that residual - and a reference evaluated with uv_star := uv_old (dt_eff := dt) moves the
    momentum columns by about 300 x the tolerance at the least over both forms and the three integrators (289 x and 287 x
    where it was chosen, 332 x and 329 x on the host of the MI355X run: the yardstick is a float32 computation of the host CPU); with
    randn alone and dt / 1.5 it would be 11 x and 17 x.  On cyl_cavity_b2 the two are about 1e5 x."""
    g = torch.Generator().manual_seed(seed)
    uv_old = uv_old.to(torch.float32)
    uv_star = (uv_old + 10.0 * torch.randn(uv_old.shape, generator=g)).to(torch.float32).contiguous()
    dt_eff = (dt.to(torch.float32).reshape(-1) / 4.0).to(torch.float32).contiguous()
    return uv_star, dt_eff
