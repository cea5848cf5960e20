"""The differentiable direct force on the GPU (csrc/direct_grad.hip, nbd.autograd.direct_accel, the simulators'
compute_accelerations() under autograd) against the fp64 closed form of tests/accel_vjp_oracle.py.

float64: inside the bar of tests/hermite_f64_oracle.py, |got - ref| <= (T + 32) 2^-53 sum|terms|, T = 8 n for a component
of the position gradient and 3 n for the mass gradient; no input is fp32-representable.
float32: on fp32-representable inputs against the same oracle; the yardstick is torch's CPU fp32 autograd through the
dense statement of the force (what a user of the reference gets), computed here, and the bars are four times
max(the yardstick's own figure, 2^-23) -- in global_rel and row_rel of the position gradient, global_rel of the mass
gradient and, elementwise, max |err| / sum|terms| of the mass gradient (relative to the value it would measure the
cancellation: torch's own per-element relative error reaches 1.5e-4 at n = 1000) -- next to the project's 1e-5 / 1e-4.
Every workspace is NaN-filled before each call. Measured on the MI355X: NOTES.md, "K-VJP"."""
import functools

import numpy as np
import pytest
import torch

import accel_vjp_oracle as vo
import hermite_f64_oracle as fo
from conftest import global_rel, load_golden, row_rel

pytestmark = pytest.mark.gpu

G, EPS = 1.0, 0.05
SIZES_F64 = [1, 2, 3, 63, 64, 65, 130, 448, 449, 1000, 5000]      # 448 / 449: one slab -> two (nbd_hermite_f64_plan)
SIZES_F32 = [1, 2, 63, 64, 65, 127, 129, 500, 2048]
U23 = 2.0 ** -23
F32, F64 = torch.float32, torch.float64


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, device, dtype=F64):
    return torch.tensor(np.asarray(a, np.float64), dtype=dtype, device=device)


def _nan_bytes(nbytes, device):
    return torch.full((nbytes // 8 + 2,), float("nan"), dtype=F64, device=device).view(torch.uint8)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _case(name, eps=EPS, fp32=False):
    """(x, m, cot, g, eps, dL/dx, dL/dm, sum|terms| of each), computed once and never written to. name: a size (Plummer,
    masses U(0.5, 1.5) / n, N(0, 1) cotangent) or a golden case (perturbed, so not fp32-representable)."""
    if isinstance(name, int):
        x, m, cot = vo.case(name, seed=200 + name, fp32=fp32)
        g = G
    else:
        gd = load_golden(name)
        x, _, m = fo.perturbed(gd["pos"], gd["vel"], gd["mass"], 5)
        cot = np.random.default_rng(6).standard_normal(x.shape)
        g, eps = float(gd["g_const"]), float(gd["softening"])
    gx, gm, sx, sm = vo.accel_vjp(x, m, cot, g, eps * eps)
    return _frozen(x, m, cot) + (g, eps) + _frozen(gx, gm, sx, sm)


@functools.lru_cache(maxsize=None)
def _yardstick(n, eps=EPS, safe_diagonal=False):
    """The figures of torch's CPU fp32 autograd through the dense statement on the fp32 case n, against the oracle:
    (global_rel and row_rel of dL/dx, global_rel of dL/dm, max |err| / sum|terms| of dL/dm). safe_diagonal: the diagonal
    of |d|^2 + eps^2 is made 1 before the power (it is zeroed after it either way), which is what keeps eps = 0 finite."""
    x, m, cot, g, eps, gx, gm, sx, sm = _case(n, eps, True)
    if safe_diagonal:
        xt = torch.tensor(x, dtype=F32, requires_grad=True)
        mt = torch.tensor(m, dtype=F32, requires_grad=True)
        d = xt.unsqueeze(0) - xt.unsqueeze(1)
        eye = torch.eye(n, dtype=torch.bool)
        w = (d.pow(2).sum(-1) + eps ** 2).masked_fill(eye, 1.0).pow(-1.5).masked_fill(eye, 0.0)
        (g * (w.unsqueeze(-1) * d * mt.view(1, n, 1)).sum(1)).backward(torch.tensor(cot, dtype=F32))
        tx, tm = xt.grad.double().numpy(), mt.grad.double().numpy()
    else:
        tx, tm = vo.torch_vjp(x, m, cot, g, eps, F32)
    return _figures(tx, tm, gx, gm, sm)


def _figures(px, pm, gx, gm, sm):
    live = sm > 0
    elem = float((np.abs(pm - gm)[live] / sm[live]).max()) if live.any() else 0.0
    return global_rel(px, gx), row_rel(px, gx), global_rel(pm, gm), elem


def _vjp64(x, m, cot, g, eps2, device, slabs=0, fill=float("nan")):
    from nbd import direct
    n = x.shape[0]
    posd, cotd = direct.alloc_rows_f64(n, device), direct.alloc_rows_f64(n, device)
    direct.hermite_f64_pack(_dev(x, device), _dev(cot, device), _dev(m, device), posd, cotd)
    ws = direct.accel_vjp_f64_workspace(n, device, slabs)
    ws.view(F64).fill_(fill)
    gp, gm = direct.accel_vjp_f64(posd, cotd, n, eps2, g, workspace=ws, slabs=slabs)
    return gp, gm


def _vjp32(x, m, cot, g, eps2, device, fill=float("nan")):
    from nbd import direct
    n = x.shape[0]
    posm, cotm = direct.alloc_posm(n, device), direct.alloc_posm(n, device)
    direct.hermite_pack(_dev(x, device, F32), _dev(cot, device, F32), _dev(m, device, F32), posm, cotm)
    ws = direct.accel_vjp_workspace(n, device)
    ws.view(F32).fill_(fill)
    return direct.accel_vjp(posm, cotm, n, direct.f32(eps2), direct.f32(g), workspace=ws)


def _check64(tag, gp, gm, case):
    x, m, cot, g, eps, gx, gmass, sx, sm = case
    n = x.shape[0]
    ok_x, fx = fo.within(_np(gp), gx, 8 * n, sx)
    ok_m, fm = fo.within(_np(gm), gmass, 3 * n, sm)
    print(f"{tag}: |grad_pos - ref| / bar = {fx:.3f}, |grad_mass - ref| / bar = {fm:.3f}")
    assert ok_x and ok_m, (tag, fx, fm)


def _check32(tag, gp, gm, case, yard):
    """The project's bars and, with a yardstick, four times max(its own figure, 2^-23) in each measure."""
    x, m, cot, g, eps, gx, gmass, sx, sm = case
    ours = _figures(_np(gp).astype(np.float64), _np(gm).astype(np.float64), gx, gmass, sm)
    names = ("grad_pos global_rel", "grad_pos row_rel", "grad_mass global_rel", "grad_mass max|err|/sum|terms|")
    for k, nm in enumerate(names):
        line = f"{tag}: {nm}: ours {ours[k]:.2e}"
        if yard is not None:
            line += f", torch fp32 {yard[k]:.2e}, ratio to the bar {ours[k] / (4 * max(yard[k], U23)):.3f}"
        print(line)
    assert np.isfinite(_np(gp)).all() and np.isfinite(_np(gm)).all()
    assert ours[0] <= 1e-5 and ours[1] <= 1e-4 and ours[2] <= 1e-5, (tag, ours)
    if yard is not None:
        for k, nm in enumerate(names):
            assert ours[k] <= 4 * max(yard[k], U23), (tag, nm, ours[k], yard[k])


# ---------------------------------------------------------------- the kernels against the oracle
@pytest.mark.parametrize("name", SIZES_F64 + ["direct_plummer_n300_ragged_mass", "direct_spiral_n25"])
def test_f64_at_the_bar(gpu_device, name):
    case = _case(name)
    x, m, cot, g, eps = case[:5]
    if not isinstance(name, int):
        assert (m == 0).any() == ("ragged_mass" in name)
    gp, gm = _vjp64(x, m, cot, g, eps * eps, gpu_device)
    assert gp.dtype == F64 and gm.dtype == F64 and gp.shape == x.shape and gm.shape == m.shape
    _check64(f"f64 n={name}", gp, gm, case)
    if name == 1:
        assert not _np(gp).any() and not _np(gm).any()          # no partner: exact zeros


@pytest.mark.parametrize("n,slabs", [(130, 1), (1000, 1), (1000, 3), (5000, 64)])
def test_f64_with_an_explicit_split(gpu_device, n, slabs):
    """Several chunks per wave (both LDS buffers reused), waves without a chunk (130 / 1; 5000 / 64), an uneven split."""
    case = _case(n)
    x, m, cot, g, eps = case[:5]
    gp, gm = _vjp64(x, m, cot, g, eps * eps, gpu_device, slabs)
    _check64(f"f64 n={n} slabs={slabs}", gp, gm, case)


@pytest.mark.parametrize("n", SIZES_F32)
def test_f32_against_the_oracle_and_the_yardstick(gpu_device, n):
    case = _case(n, EPS, True)
    x, m, cot, g, eps = case[:5]
    for a in (x, m, cot):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    gp, gm = _vjp32(x, m, cot, g, eps * eps, gpu_device)
    assert gp.dtype == F32 and gm.dtype == F32
    _check32(f"f32 n={n}", gp, gm, case, _yardstick(n))
    if n == 1:
        assert not _np(gp).any() and not _np(gm).any()


def test_f32_n5000_against_the_oracle(gpu_device):
    """The project's bars only: the dense yardstick is too large here. 79 chunks, 40 groups."""
    case = _case(5000, EPS, True)
    x, m, cot, g, eps = case[:5]
    gp, gm = _vjp32(x, m, cot, g, eps * eps, gpu_device)
    _check32("f32 n=5000", gp, gm, case, None)


@pytest.mark.parametrize("n", [65, 130])
def test_no_self_term_leaks_at_a_tiny_softening(gpu_device, n):
    """eps = 1e-6: the un-masked path with s^3 up to 1e18 on the diagonal. A residual h_ii, or an i == j term of d . g_j,
    would miss the bars by many orders of magnitude."""
    eps = 1e-6
    case64 = _case(n, eps)
    x, m, cot, g = case64[:4]
    gp, gm = _vjp64(x, m, cot, g, eps * eps, gpu_device)
    _check64(f"f64 n={n} eps=1e-6", gp, gm, case64)
    case32 = _case(n, eps, True)
    x, m, cot, g = case32[:4]
    gp, gm = _vjp32(x, m, cot, g, eps * eps, gpu_device)
    _check32(f"f32 n={n} eps=1e-6", gp, gm, case32, _yardstick(n, eps))


@pytest.mark.parametrize("n", [64, 130])
def test_zero_softening_is_the_closed_form_over_the_other_bodies(gpu_device, n):
    """eps = 0 (every chunk index-masked): finite, and the sum over j != i. torch's autograd through the plain dense
    statement gives NaN here; the fp32 yardstick is the statement with the diagonal kept finite."""
    case64 = _case(n, 0.0)
    x, m, cot, g = case64[:4]
    assert np.unique(x, axis=0).shape[0] == n
    gp, gm = _vjp64(x, m, cot, g, 0.0, gpu_device)
    assert torch.isfinite(gp).all() and torch.isfinite(gm).all()
    _check64(f"f64 n={n} eps=0", gp, gm, case64)
    case32 = _case(n, 0.0, True)
    x, m, cot, g = case32[:4]
    assert np.unique(x, axis=0).shape[0] == n
    assert np.isnan(vo.torch_vjp(x, m, cot, g, 0.0, F32)[0]).all()
    gp, gm = _vjp32(x, m, cot, g, 0.0, gpu_device)
    _check32(f"f32 n={n} eps=0", gp, gm, case32, _yardstick(n, 0.0, True))


def test_translation_invariance(gpu_device):
    """sum_i dL/dx_i = 0: the pair terms are antisymmetric. Each row is within bar(8 n, its sum|terms|) of its exact value
    and the fp64 sum of the n rows adds at most n 2^-53 sum|rows| <= n 2^-53 sum of all |terms|: T = 9 n over the
    summed |terms|."""
    n = 4096
    case = _case(n)
    x, m, cot, g, eps, gx, gmass, sx, sm = case
    gp, gm = _vjp64(x, m, cot, g, eps * eps, gpu_device)
    total = _np(gp).sum(0)
    b = fo.bar(9 * n, sx.sum(0))
    print(f"translation invariance: |sum| / bar = {(np.abs(total) / b).max():.3f}")
    assert np.all(np.abs(total) <= b)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_deterministic_with_any_workspace(gpu_device, dtype):
    """Two calls whose workspaces hold different things give the same bits."""
    case = _case(1000, EPS, dtype == F32)
    x, m, cot, g, eps = case[:5]
    run = _vjp32 if dtype == F32 else _vjp64
    a = run(x, m, cot, g, eps * eps, gpu_device, fill=float("nan"))
    b = run(x, m, cot, g, eps * eps, gpu_device, fill=-3.25e7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------- the autograd surface
def _sim(dtype, x, v, m, **kw):
    from galaxify import simulation
    kw.setdefault("g_const", G); kw.setdefault("softening", EPS); kw.setdefault("calc_energy", False)
    if dtype == F64:
        return simulation.HermiteSimulator(positions=x, velocities=v, masses=m, device="cuda", dtype=F64, **kw)
    return simulation.LeapFrogSimulator(positions=x, velocities=v, masses=m, device="cuda", **kw)


def _state(n, seed, dtype):
    x, m, cot = vo.case(n, seed=seed, fp32=dtype == F32)
    v = np.random.default_rng(seed + 1).standard_normal((n, 3)) * 0.3
    return x, v, m, cot


@pytest.mark.parametrize("dtype", [F32, F64])
def test_forward_is_the_simulators_acceleration(gpu_device, dtype):
    from nbd import autograd
    x, v, m, _ = _state(300, 41, dtype)
    sim = _sim(dtype, x, v, m, g_const=1.5, softening=0.07)
    ref = sim.compute_accelerations()
    assert ref.grad_fn is None and not ref.requires_grad                        # nothing requires grad: today's path
    a = autograd.direct_accel(sim.positions, sim.masses, 1.5, 0.07)
    assert a.dtype == dtype and torch.equal(a, ref) and a.grad_fn is None
    sim.positions.requires_grad_()
    b = sim.compute_accelerations()
    assert b.grad_fn is not None and torch.equal(b, ref)
    with torch.no_grad():
        c = sim.compute_accelerations()
    assert c.grad_fn is None and not c.requires_grad and torch.equal(c, ref)    # no graph under no_grad
    sim.positions.requires_grad_(False)
    sim.masses.requires_grad_()
    assert sim.compute_accelerations().grad_fn is not None


@pytest.mark.parametrize("n", [5, 67])
def test_gradcheck_float64(gpu_device, n):
    from nbd import autograd
    x, m, _ = vo.case(n, seed=50 + n)
    xt = _dev(x, gpu_device).requires_grad_()
    mt = _dev(m, gpu_device).requires_grad_()
    assert torch.autograd.gradcheck(lambda p, q: autograd.direct_accel(p, q, 1.3, 0.2), (xt, mt))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_backward_once_and_only_what_is_asked(gpu_device, dtype):
    from nbd import autograd
    x, v, m, cot = _state(130, 61, dtype)
    xt, mt, ct = (_dev(a, gpu_device, dtype) for a in (x, m, cot))
    xg, mg = xt.clone().requires_grad_(), mt.clone().requires_grad_()
    a = autograd.direct_accel(xg, mg, G, EPS)
    a.backward(ct)
    with pytest.raises(RuntimeError):
        a.backward(ct)                                                           # once: the packed copy is released
    # against the kernels driven directly, bit for bit
    run = _vjp32 if dtype == F32 else _vjp64
    gp, gm = run(x, m, cot, G, EPS * EPS, gpu_device)
    assert torch.equal(xg.grad, gp) and torch.equal(mg.grad, gm)
    # only positions, only masses
    xo = xt.clone().requires_grad_()
    a = autograd.direct_accel(xo, mt, G, EPS)
    assert a.grad_fn.next_functions[1][0] is None
    a.backward(ct)
    assert torch.equal(xo.grad, gp) and mt.grad is None
    mo = mt.clone().requires_grad_()
    a = autograd.direct_accel(xt, mo, G, EPS)
    assert a.grad_fn.next_functions[0][0] is None
    a.backward(ct)
    assert torch.equal(mo.grad, gm) and xt.grad is None
    # a non-contiguous cotangent
    xs = xt.clone().requires_grad_()
    wide = torch.zeros((130, 6), dtype=dtype, device=gpu_device)
    wide[:, ::2] = ct
    assert not wide[:, ::2].is_contiguous()
    autograd.direct_accel(xs, mt, G, EPS).backward(wide[:, ::2])
    assert torch.equal(xs.grad, gp)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_state_is_snapshotted_at_the_forward(gpu_device, dtype):
    """step() writes positions through raw pointers, which torch's version counters do not see: the node must have
    packed its own copy."""
    from nbd import autograd
    x, v, m, cot = _state(200, 71, dtype)
    sim = _sim(dtype, x, v, m, dt=0.05)
    ct = _dev(cot, gpu_device, dtype)
    sim.positions.requires_grad_()
    sim.masses.requires_grad_()
    x0, m0 = sim.positions.detach().clone(), sim.masses.detach().clone()
    a = sim.compute_accelerations()
    sim.step()
    sim.step()
    assert not torch.equal(sim.positions.detach(), x0)
    a.backward(ct)
    xf, mf = x0.clone().requires_grad_(), m0.clone().requires_grad_()
    autograd.direct_accel(xf, mf, G, EPS).backward(ct)
    assert torch.equal(sim.positions.grad, xf.grad) and torch.equal(sim.masses.grad, mf.grad)


def test_three_leapfrog_steps_compose(gpu_device):
    """A kick-drift-kick rollout in torch ops around direct_accel, float64, n = 33: d sum(x_final^2) / d (v0, m) against
    CPU fp64 autograd of the dense statement, to 1e-10 global_rel (loose against the fp64 sum bars over three steps;
    the measured figure is in NOTES.md)."""
    from nbd import autograd
    n, dt, g, eps = 33, 0.02, 1.0, 0.05
    x, v, m, _ = _state(n, 81, F64)

    def rollout(force, x0, v0, mm):
        xx, vv = x0, v0
        a = force(xx, mm)
        for _ in range(3):
            vv = vv + 0.5 * dt * a
            xx = xx + dt * vv
            a = force(xx, mm)
            vv = vv + 0.5 * dt * a
        return (xx * xx).sum()

    grads = []
    for device, force in ((gpu_device, lambda p, q: autograd.direct_accel(p, q, g, eps)),
                          ("cpu", lambda p, q: vo.dense_accel(p, q, g, eps))):
        x0 = torch.tensor(x, dtype=F64, device=device)
        v0 = torch.tensor(v, dtype=F64, device=device, requires_grad=True)
        mm = torch.tensor(m, dtype=F64, device=device, requires_grad=True)
        rollout(force, x0, v0, mm).backward()
        grads.append((_np(v0.grad), _np(mm.grad)))
    ev, em = global_rel(grads[0][0], grads[1][0]), global_rel(grads[0][1], grads[1][1])
    print(f"three leapfrog steps: d/dv0 {ev:.2e}, d/dm {em:.2e}")
    assert ev <= 1e-10 and em <= 1e-10


def test_sharded_simulator_refuses(gpu_device, tmp_path, monkeypatch):
    import torch.distributed as dist
    x, v, m, _ = _state(300, 91, F32)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1)
    try:
        monkeypatch.setenv("NBD_FORCE_SHARDED", "1")
        sim = _sim(F32, x, v, m, process_group=dist.group.WORLD)
        monkeypatch.delenv("NBD_FORCE_SHARDED")
        assert sim._sharded
        assert sim.compute_accelerations().grad_fn is None
        sim.positions.requires_grad_()
        with pytest.raises(ValueError, match="process_group is not supported"):
            sim.compute_accelerations()
        with torch.no_grad():
            assert sim.compute_accelerations().grad_fn is None
    finally:
        dist.destroy_process_group()
