"""run()'s captured-chunk engine (galaxify/simulation.py, _ChunkedRun) without a GPU: which integrator classes may
replay a captured step, and how a host copy of a batch's chunk buffer becomes SimulationStates."""
import pytest
import torch

from galaxify import simulation


def test_capturable_is_a_class_level_predicate():
    """A class replays captured chunks only when the class that defines its step() also defines the in-place step: an
    overriding step() must never be replaced by its parent's captured one."""
    for cls in (simulation.LeapFrogSimulator, simulation.EulerSimulator, simulation.HermiteSimulator):
        assert cls._capturable(), cls.__name__
    for cls in (simulation.BaseSimulator, simulation.BlockHermiteSimulator):
        assert not cls._capturable(), cls.__name__

    class Inherits(simulation.LeapFrogSimulator):
        pass

    class OverridesStep(simulation.LeapFrogSimulator):
        def step(self):
            super().step()

    class OverridesBoth(OverridesStep):
        def step(self):
            super().step()

        def _step_in_place(self):
            super()._step_in_place()

    assert Inherits._capturable() and not OverridesStep._capturable() and OverridesBoth._capturable()
    assert simulation.HermiteSimulator._carried == (("accelerations", "_acc_g"), ("jerks", "_jerk_g"))
    assert simulation.LeapFrogSimulator._carried == simulation.EulerSimulator._carried == (("accelerations", "_acc_g"),)


@pytest.mark.parametrize("calc_energy", [True, False])
def test_batch_states_from_a_hand_filled_chunk_buffer(calc_energy):
    """Two scenes, 3 bodies and none, 2 steps: ring (m, 3, N, 3) fp32, then from the next multiple of 16 bytes the
    energies (m, S, 2) fp64. N = 3 makes the ring 216 bytes, so the energies start at 224: the padding is exercised."""
    m, offsets = 2, [0, 3, 3]
    ring_b, uk_at, size = simulation._batch_chunk_layout(m, 3, 2)
    assert (ring_b, uk_at, size) == (216, 224, 224 + 64)
    host = torch.full((size,), 0xFF, dtype=torch.uint8)
    ring = torch.arange(m * 27, dtype=torch.float32).view(m, 3, 3, 3)
    uk = torch.tensor([[[-1.5, 0.25], [0.0, 0.0]], [[-2.5, 0.75], [0.0, 0.0]]], dtype=torch.float64)
    host[:ring_b] = ring.view(-1).view(torch.uint8)
    host[uk_at:] = uk.view(-1).view(torch.uint8)
    out = [[], []]
    simulation._batch_states(host, m, offsets, calc_energy, 40, [1e-5, 2e-5], out)
    assert [len(o) for o in out] == [m, m]
    for s in range(m):
        a, b = out[0][s], out[1][s]
        assert (a.step, b.step) == (40 + s, 40 + s) and a.step_time == b.step_time == [1e-5, 2e-5][s]
        for k, name in enumerate(("positions", "velocities", "accelerations")):
            assert torch.equal(getattr(a, name), ring[s, k]) and getattr(b, name).shape == (0, 3)
        if calc_energy:
            assert (a.u_energy, a.k_energy) == tuple(uk[s, 0].tolist()) and (b.u_energy, b.k_energy) == (0.0, 0.0)
        else:
            assert a.u_energy is a.k_energy is b.u_energy is b.k_energy is None
    # views of the host buffer, not copies
    host[:4] = torch.tensor([7.0], dtype=torch.float32).view(torch.uint8)
    assert float(out[0][0].positions[0, 0]) == 7.0
