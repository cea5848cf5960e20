"""Consistent-potential diagnostics on the MI355X (csrc/direct_diag.hip): per-body potentials and the invariants row
against the fp64 oracle (tests/diag_oracle.py) over the chunk / workgroup / slab edges, determinism, the energy error of
the Hermite integrator measured with them (where the reference-convention U + K says nothing), run() with
calc_invariants on the eager and the captured path, BatchedSimulator bit-identical to lone simulators, and the refusal
of a range-sharded simulator.

Every test prints its figure before it asserts (run with -s); NOTES.md, "Consistent-potential diagnostics", holds the
measurements."""
import functools

import numpy as np
import pytest
import torch

import diag_oracle as do
import hermite_oracle as ho
from conftest import load_golden

pytestmark = pytest.mark.gpu

# chunk (64) and workgroup (128) edges, the padded tail, ragged masses (300), several slabs, 130 chunks split unevenly
# over the waves (8257)
SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 300, 1000, 4096, 8257]
SOFTENINGS = [0.05, 0.0]
PHI_TOL = 5e-6          # ~6 roundings of the pair term + a 63-add fp32 chain of same-signed terms: 70 * 2^-24 = 4.2e-6
SUM_TOL = 1e-12         # fp64 sums of identical terms in another order, against the sum of |terms|


def _f32(x):
    return float(np.float32(x))


@functools.lru_cache(maxsize=None)
def _system(n):
    """(pos, vel, mass) fp32 arrays, read-only."""
    if n == 300:
        g = load_golden("direct_plummer_n300_ragged_mass")
        out = tuple(np.asarray(g[k], np.float32) for k in ("pos", "vel", "mass"))
    else:
        from nbd.plummer import generate_plummer
        out = tuple(np.asarray(t, np.float32) for t in generate_plummer(n, seed=100 + n))
    for a in out:
        a.setflags(write=False)
    return out


def _shifted():
    """A system far from the origin with a bulk velocity: C, P and L far from zero."""
    p, v, m = _system(129)
    return (p + np.float32([100.0, 0.0, 0.0])).astype(np.float32), (v + np.float32([0.3, -0.2, 0.1])).astype(np.float32), m


@functools.lru_cache(maxsize=None)
def _oracle(key, eps):
    p, v, m = _shifted() if key == "shifted" else _system(key)
    phi = do.potentials(p, m, 1.0, _f32(eps * eps))
    sums, abs_sums = do.sums(p, v, m, phi)
    return phi, do.invariants_row(p, v, m, phi), abs_sums


def _sim(key, eps, cls="LeapFrogSimulator", **kw):
    from galaxify import simulation
    p, v, m = _shifted() if key == "shifted" else _system(key)
    return getattr(simulation, cls)(positions=p, velocities=v, masses=m, g_const=1.0, softening=eps, dt=0.01,
                                    calc_energy=False, device="cuda", **kw)


@pytest.mark.parametrize("eps", SOFTENINGS)
@pytest.mark.parametrize("n", SIZES)
def test_potentials_match_f64_oracle(n, eps, gpu_device):
    sim = _sim(n, eps)
    phi = sim.compute_potentials()
    assert phi.dtype == torch.float64 and tuple(phi.shape) == (n,) and phi.is_cuda
    phi = phi.cpu().numpy()
    ref = _oracle(n, eps)[0]
    err = np.abs(phi - ref)
    rel = float((err / np.maximum(np.abs(ref), 1e-300)).max()) if n > 1 else float(err.max())
    print(f"phi n={n} eps={eps}: max per-body relative error {rel:.3e}")
    assert np.isfinite(phi).all()
    assert (err <= PHI_TOL * np.abs(ref)).all(), rel


def _check_row(row, key, eps):
    _, ref, abs_sums = _oracle(key, eps)
    M = ref[0]
    bound = np.empty(11)
    bound[0] = SUM_TOL * abs_sums[0]
    bound[1:4] = SUM_TOL * abs_sums[1:4] / M
    bound[4:11] = SUM_TOL * abs_sums[4:11]
    err = np.abs(row[:11] - ref[:11])
    print(f"row {key} eps={eps}: max err/bound of M,C,P,L,K {float((err / np.maximum(bound, 1e-300)).max()):.3e}; "
          f"U rel {abs(row[11] - ref[11]) / max(abs(ref[11]), 1e-300):.3e}, "
          f"E rel {abs(row[12] - ref[12]) / max(abs(ref[12]), 1e-300):.3e}")
    assert (err <= bound).all(), (err, bound)
    assert abs(row[11] - ref[11]) <= PHI_TOL * abs(ref[11])
    assert abs(row[12] - ref[12]) <= PHI_TOL * abs(ref[12])
    assert row[12] == row[10] + row[11]
    assert row[13] == (-2.0 * row[10] / row[11] if row[11] != 0 else 0.0)
    assert row[14] == 0.0 and row[15] == 0.0


@pytest.mark.parametrize("eps", SOFTENINGS)
@pytest.mark.parametrize("key", SIZES + ["shifted"])
def test_invariants_row_matches_f64_oracle(key, eps, gpu_device):
    from nbd import direct
    sim = _sim(key, eps)
    phi = sim.compute_potentials()
    row = direct.invariants(sim._posm, sim.velocities, phi, sim.n).cpu().numpy()
    _check_row(row, key, eps)
    inv = sim.compute_invariants()
    assert inv.row() == row.tolist()
    if key == "shifted":
        assert abs(inv.com[0]) > 99 and abs(inv.momentum[0]) > 0.2 and abs(inv.angular_momentum[2]) > 10


def test_empty_system(gpu_device):
    from galaxify import simulation
    z = np.zeros((0, 3))
    sim = simulation.HermiteSimulator(positions=z, velocities=z, masses=np.zeros(0), device="cuda", calc_energy=False,
                                      calc_invariants=True)
    phi = sim.compute_potentials()
    assert tuple(phi.shape) == (0,) and phi.dtype == torch.float64
    assert sim.compute_invariants().row() == [0.0] * 16
    assert [s.invariants.row() for s in sim.run(2)] == [[0.0] * 16] * 2


@pytest.mark.parametrize("n,eps", [(129, 0.0), (1000, 0.05), (8257, 0.05)])
def test_two_calls_are_bit_identical(n, eps, gpu_device):
    sim = _sim(n, eps)
    phi_a, inv_a = sim.compute_potentials(), sim.compute_invariants()
    phi_b, inv_b = sim.compute_potentials(), sim.compute_invariants()
    assert torch.equal(phi_a, phi_b) and inv_a == inv_b
    other = _sim(n, eps, cls="HermiteSimulator")                # another simulator, other buffers
    assert torch.equal(other.compute_potentials(), phi_a) and other.compute_invariants() == inv_a


def test_rectangular_potential_matches_the_square_one(gpu_device):
    """Targets [lo, hi) of the system against all sources, with their offset: the rows of the square call's sums, to
    fp64 rounding (another slab split), and the pair j == offset + i is the one excluded."""
    from nbd import direct
    n, lo, hi = 1000, 130, 777
    sim = _sim(n, 0.05)
    full = sim.compute_potentials()
    part = direct.potential(sim._posm, n, sim._posm[lo:hi], hi - lo, lo, sim._eps2, sim._g)
    assert float(((part - full[lo:hi]).abs() / full[lo:hi].abs()).max()) <= 1e-12
    ref = _oracle(n, 0.05)[0][lo:hi]
    assert (np.abs(part.cpu().numpy() - ref) <= PHI_TOL * np.abs(ref)).all()


# ------------------------------------------------------------------ the energy error means something
def _oracle_drift(x, v, m, dt, eps2, steps):
    """max |E - E0| / |E0| of the fp64 Hermite run of the same steps, E = K + 1/2 sum m phi."""
    x = np.asarray(x, np.float32).astype(np.float64); v = np.asarray(v, np.float32).astype(np.float64)
    m = np.asarray(m, np.float32).astype(np.float64)

    def energy(x, v):
        phi = _phi64(x, m, eps2)
        return float((0.5 * m * (v * v).sum(1)).sum() + 0.5 * (m * phi).sum())
    a, j = ho.accel_jerk(x, v, m, 1.0, eps2)
    e0 = energy(x, v)
    worst = 0.0
    for _ in range(steps):
        x, v, a, j = ho.hermite_step(x, v, a, j, m, dt, 1.0, eps2)
        worst = max(worst, abs(energy(x, v) - e0) / abs(e0))
    return worst


def _phi64(x, m, eps2):
    """The oracle's potential of an fp64 state (no rounding of the state to fp32)."""
    d = x[None, :, :] - x[:, None, :]
    r2 = (d * d).sum(-1) + eps2
    np.fill_diagonal(r2, 1.0)
    s = 1.0 / np.sqrt(r2)
    np.fill_diagonal(s, 0.0)
    return -(m[None, :] * s).sum(1)


def _drifts(sim, steps):
    """(consistent, reference-convention) max |E - E0| / |E0| over the states of run(steps)."""
    e0 = sim.compute_invariants().energy
    u0, k0 = sim.compute_energies()
    states = sim.run(steps)
    assert len(states) == steps and all(s.invariants is not None for s in states)
    good = max(abs(s.invariants.energy - e0) for s in states) / abs(e0)
    naive = max(abs(s.u_energy + s.k_energy - (u0 + k0)) for s in states) / abs(u0 + k0)
    return good, naive


def test_two_body_energy_error_is_the_integrators(gpu_device):
    """two_body(0.5), eps = 0.1, one period in 128 Hermite steps: the drift of E = K + 1/2 sum m phi stays within twice the
    fp64 oracle's drift of the same steps (truncation error dominates fp32 round-off ~50x here), while the reference
    convention's U + K swings by half of |E|."""
    from galaxify import simulation
    x0, v0, m, period = ho.two_body(0.5)
    eps, steps = 0.1, 128
    dt = period / steps
    ref = _oracle_drift(x0, v0, m, dt, _f32(eps * eps), steps)
    sim = simulation.HermiteSimulator(positions=x0, velocities=v0, masses=m, g_const=1.0, softening=eps, dt=dt,
                                      calc_energy=True, device="cuda", calc_invariants=True)
    good, naive = _drifts(sim, steps)
    print(f"two-body: consistent drift {good:.3e} (fp64 oracle {ref:.3e}), reference-convention swing {naive:.3e}")
    assert 3e-5 < ref < 1.3e-4                       # the oracle run itself (6.4e-5)
    assert good <= 2.0 * ref
    assert naive >= 0.1


def test_plummer_consistent_drift_is_100x_below_the_reference_convention(gpu_device):
    from galaxify import simulation
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(256, seed=5)
    sim = simulation.HermiteSimulator(positions=p, velocities=v, masses=m, g_const=1.0, softening=0.05, dt=1.0 / 64,
                                      calc_energy=True, device="cuda", calc_invariants=True)
    good, naive = _drifts(sim, 64)
    print(f"plummer 256: consistent drift {good:.3e}, reference-convention drift {naive:.3e}")
    assert 100.0 * good <= naive


# ------------------------------------------------------------------ run()
RUN_CASES = [("LeapFrogSimulator", {}, True), ("LeapFrogSimulator", {}, False), ("HermiteSimulator", {}, True),
             ("HermiteSimulator", {}, False), ("BlockHermiteSimulator", {"max_level": 3}, False)]


@pytest.mark.parametrize("cls,extra,graph", RUN_CASES)
def test_run_carries_the_invariants_of_every_state(cls, extra, graph, gpu_device, monkeypatch):
    from galaxify import simulation
    p, v, m = _system(129)
    kw = dict(positions=p, velocities=v, masses=m, g_const=1.0, softening=0.05, dt=0.01, calc_energy=True,
              device="cuda", **extra)
    if not graph:
        monkeypatch.setenv("NBD_RUN_GRAPH", "0")
    make = getattr(simulation, cls)
    on, off, twin = make(calc_invariants=True, **kw), make(**kw), make(**kw)
    assert on._graph_run_ok(16) == (graph and cls != "BlockHermiteSimulator")
    s_on, s_off = on.run(16), off.run(16)
    assert len(s_on) == len(s_off) == 16
    for k in range(16):
        twin.step()
        assert s_on[k].invariants == twin.compute_invariants(), k
        assert s_off[k].invariants is None
        assert torch.equal(s_on[k].positions, s_off[k].positions) and torch.equal(s_on[k].velocities, s_off[k].velocities)
        assert torch.equal(s_on[k].accelerations, s_off[k].accelerations)
        assert (s_on[k].u_energy, s_on[k].k_energy) == (s_off[k].u_energy, s_off[k].k_energy)
        assert torch.equal(s_on[k].positions, twin.positions.cpu())


# ------------------------------------------------------------------ batched
def _scenes():
    from galaxify import galaxies
    from nbd.plummer import generate_plummer

    def plummer(n, seed, g, eps, dt):
        p, v, m = generate_plummer(n, seed=seed)
        return dict(pos=p, vel=v, mass=m, g=g, eps=eps, dt=dt)

    def spiral(n, seed):
        p, v, m = galaxies.generate_spiral(n_bodies=n, total_mass=1.0, radial_scale=3.0, height_scale=0.3,
                                           g_const=4.5e-6, black_hole_mass=0.01, seed=seed)
        return dict(pos=p, vel=v, mass=m, g=4.5e-6, eps=0.05, dt=1e-4)
    return [spiral(3, 4), plummer(64, 3, 1.0, 0.0, 1e-3), spiral(25, 2), plummer(129, 5, 2.0, 0.02, 1e-3),
            plummer(300, 7, 1.0, 0.1, 2e-3), spiral(500, 3)]


def _batch(scenes, integrator, **kw):
    from galaxify import simulation
    return simulation.BatchedSimulator(systems=[(s["pos"], s["vel"], s["mass"]) for s in scenes], integrator=integrator,
                                       g_const=[s["g"] for s in scenes], softening=[s["eps"] for s in scenes],
                                       dt=[s["dt"] for s in scenes], device="cuda", **kw)


def _assert_scenes_equal_lone(sim, scenes, what):
    from galaxify import simulation
    phi = sim.compute_potentials()
    invs = sim.compute_invariants()
    assert phi.dtype == torch.float64 and tuple(phi.shape) == (sim.n,) and len(invs) == len(scenes)
    for i, s in enumerate(scenes):
        lo, hi = int(sim.offsets[i]), int(sim.offsets[i + 1])
        lone = simulation.LeapFrogSimulator(positions=sim.positions[lo:hi], velocities=sim.velocities[lo:hi],
                                            masses=sim.masses[lo:hi], g_const=s["g"], softening=s["eps"], dt=s["dt"],
                                            calc_energy=False, device="cuda")
        assert torch.equal(phi[lo:hi], lone.compute_potentials()), (what, i)
        assert invs[i] == lone.compute_invariants(), (what, i)


@pytest.mark.parametrize("integrator", ["leapfrog", "hermite"])
def test_batched_scenes_are_bit_identical_to_lone_simulators(integrator, gpu_device):
    scenes = _scenes()
    assert [s["pos"].shape[0] for s in scenes] == [3, 64, 25, 129, 300, 500]
    assert len({(s["g"], s["eps"]) for s in scenes}) >= 4
    sim = _batch(scenes, integrator, calc_energy=False)
    _assert_scenes_equal_lone(sim, scenes, "construction")
    for _ in range(3):
        sim.step()
    _assert_scenes_equal_lone(sim, scenes, "after 3 steps")


@pytest.mark.parametrize("integrator", ["leapfrog", "hermite"])
def test_batched_captured_run_equals_eager_steps(integrator, gpu_device):
    """19 steps: two captured chunks of 8, then an eager tail of 3."""
    scenes = _scenes()
    empty = dict(pos=np.zeros((0, 3)), vel=np.zeros((0, 3)), mass=np.zeros(0), g=1.0, eps=0.1, dt=0.01)
    scenes = scenes[:2] + [empty] + scenes[2:]
    ran = _batch(scenes, integrator, calc_energy=True, calc_invariants=True)
    plain = _batch(scenes, integrator, calc_energy=True)
    eager = _batch(scenes, integrator, calc_energy=False)
    assert ran._chunk_len() >= 8
    out, out_plain = ran.run(19), plain.run(19)
    for k in range(19):
        eager.step()
        invs = eager.compute_invariants()
        for i in range(len(scenes)):
            st, sp = out[i][k], out_plain[i][k]
            assert st.invariants == invs[i], (k, i)
            assert sp.invariants is None
            assert torch.equal(st.positions, sp.positions) and torch.equal(st.velocities, sp.velocities), (k, i)
            assert (st.u_energy, st.k_energy) == (sp.u_energy, sp.k_energy), (k, i)
    assert out[2][0].invariants.row() == [0.0] * 16


def test_range_sharded_simulator_refuses(gpu_device, tmp_path, monkeypatch):
    import torch.distributed as dist
    from galaxify import simulation
    p, v, m = _system(300)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        monkeypatch.setenv("NBD_FORCE_SHARDED", "1")
        sim = simulation.LeapFrogSimulator(positions=p, velocities=v, masses=m, device="cuda", calc_energy=False,
                                           process_group=dist.group.WORLD)
        monkeypatch.delenv("NBD_FORCE_SHARDED")
        assert sim._sharded
        with pytest.raises(ValueError):
            sim.compute_potentials()
        with pytest.raises(ValueError):
            sim.compute_invariants()
    finally:
        dist.destroy_process_group()
