"""Scene-by-scene run() against one batched run() (galaxify.simulation.BatchedSimulator) for the dataset shapes of the
direct integrator; prints ONE JSON line. Cases:
  six   : the reference experiment drivers' six scenes (3, 25, 50, 100, 250, 500 bodies) x 1000 steps, energies on;
  many  : 1024 scenes x 100 bodies x 100 steps, energies on (scene by scene timed on the first --sample scenes and
          scaled to 1024: the per-scene cost does not depend on the scene's index);
  large : 4 scenes x 16 384 bodies x 100 steps, energies off (pair rate: large scenes must not be penalised).
Times are wall clock around run() after a warm-up run() of the same length (graph capture excluded on both sides), and
GPU time = the sum of SimulationState.step_time (the batched step's GPU time is spread over its S scenes).
--integrator hermite compares scene-by-scene HermiteSimulator.run() with one batched Hermite run(), and adds the batched
leapfrog time of the same scenes from the same process (batched_leapfrog_*, hermite_over_leapfrog_gpu).
--integrator hermite --dtype float64 compares scene-by-scene HermiteSimulator(dtype=torch.float64).run() (eager: the
one-system float64 step has no captured form) with one batched float64 run(), and adds the batched float32 Hermite time
of the same scenes from the same process (batched_f32_hermite_*, f64_over_f32_gpu). --out FILE also writes the line there
(profiles/r17_batch_hermite_f64.json is this tool's output for float64).
--integrator hermite6 (float64 implied) compares scene-by-scene Hermite6Simulator.run() (eager) with one batched 6th-order
run(), and adds the batched float64 4th-order time of the same scenes from the same process (batched_f64_hermite_*,
hermite6_over_hermite_gpu); profiles/r21_batch_hermite6.json holds two runs' lines.
--integrator block_hermite / block_hermite6 (float64 implied; --eta, --max-level) compares scene-by-scene
BlockHermiteSimulator(dtype=torch.float64).run() resp. BlockHermite6Simulator.run() with one batched block run(), and adds
the block-step counts of the timed runs: the sum of the scenes' own (scene_block_steps), the ensemble's
(ensemble_block_steps, the size of the union of the scenes' tick sets), their ratio and the batched GPU time per ensemble
block step; profiles/r24_batch_block.json holds both orders' lines.

  python tools/bench_direct_scenes.py [--sample 128] [--cases six,many,large] [--integrator leapfrog|hermite|hermite6|
                                      block_hermite|block_hermite6] [--dtype float32|float64] [--eta 0.02]
                                      [--max-level 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nbody-deep-sim_amd"))

import torch  # noqa: E402
from galaxify import galaxies, simulation  # noqa: E402

G, EPS, DT = 4.5e-6, 0.05, 1e-4


def spiral(n, seed):
    return galaxies.generate_spiral(n_bodies=n, total_mass=1.0, radial_scale=3.0, height_scale=0.3, g_const=G,
                                    black_hole_mass=0.01, seed=seed)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def batched(systems, steps, energy, integrator, **kw):
    """(wall s, GPU s, block steps) of one batched run() after a warm-up run() of the same length. kw: dtype=torch.float64,
    and eta, max_level for the block integrators (block steps: the ensemble's in the timed run; 0 for the others)."""
    bat = simulation.BatchedSimulator(systems=systems, integrator=integrator, g_const=G, softening=EPS, dt=DT,
                                      calc_energy=energy, device="cuda", **kw)
    bat.run(steps)
    before = bat.block_steps
    wall, runs = timed(lambda: bat.run(steps))
    return wall, sum(st.step_time for r in runs for st in r), bat.block_steps - before


BLOCK = {"block_hermite": simulation.BlockHermiteSimulator, "block_hermite6": simulation.BlockHermite6Simulator}


def case(sizes, steps, energy, sample=None, integrator="leapfrog", dtype=torch.float32, block_kw=None):
    systems = [spiral(n, 1 + i) for i, n in enumerate(sizes)]
    seq = systems if sample is None else systems[:sample]
    cls = {"hermite": simulation.HermiteSimulator, "hermite6": simulation.Hermite6Simulator, **BLOCK}.get(
        integrator, simulation.LeapFrogSimulator)
    kw = {} if dtype == torch.float32 else {"dtype": dtype}           # (only the Hermite classes take the keyword)
    if integrator in BLOCK:
        kw.update(block_kw)                                           # eta, max_level: the same for both sides
    sims = [cls(positions=p, velocities=v, masses=m, g_const=G, softening=EPS, dt=DT, calc_energy=energy, device="cuda",
                **kw) for p, v, m in seq]
    for s in sims:
        s.run(steps)                                      # warm-up: captures
    own_before = sum(getattr(s, "block_steps", 0) for s in sims)
    wall_seq, runs = timed(lambda: [s.run(steps) for s in sims])
    own_steps = sum(getattr(s, "block_steps", 0) for s in sims) - own_before
    gpu_seq = sum(st.step_time for r in runs for st in r)
    scale = len(systems) / len(seq)
    wall_bat, gpu_bat, union_steps = batched(systems, steps, energy, integrator, **kw)
    pairs = sum(n * n for n in sizes) * steps
    out = {} if integrator == "leapfrog" else {"integrator": integrator}
    if kw:
        out["dtype"] = str(dtype).replace("torch.", "")
    if integrator in BLOCK:
        out.update(block_kw)
    out.update({"scenes": len(sizes), "bodies": sum(sizes), "steps": steps, "energy": energy,
                "scene_by_scene_sampled": len(seq),
                "scene_by_scene_wall_us_per_step": 1e6 * wall_seq * scale / steps,
                "scene_by_scene_gpu_us_per_step": 1e6 * gpu_seq * scale / steps,
                "batched_wall_us_per_step": 1e6 * wall_bat / steps,
                "batched_gpu_us_per_step": 1e6 * gpu_bat / steps,
                "speedup_wall": wall_seq * scale / wall_bat, "speedup_gpu": gpu_seq * scale / gpu_bat,
                "batched_gpairs_per_s_gpu": pairs / gpu_bat * 1e-9,
                "scene_by_scene_gpairs_per_s_gpu": pairs / (gpu_seq * scale) * 1e-9})
    if integrator in BLOCK:
        out.update({"scene_block_steps": own_steps * scale, "ensemble_block_steps": union_steps,
                    "scene_over_ensemble_block_steps": own_steps * scale / union_steps,
                    "batched_gpu_us_per_ensemble_block_step": 1e6 * gpu_bat / union_steps,
                    "scene_by_scene_gpu_us_per_block_step": 1e6 * gpu_seq / own_steps})
    elif integrator == "hermite6":
        wall_4, gpu_4, _ = batched(systems, steps, energy, "hermite", **kw)
        out.update({"batched_f64_hermite_wall_us_per_step": 1e6 * wall_4 / steps,
                    "batched_f64_hermite_gpu_us_per_step": 1e6 * gpu_4 / steps,
                    "hermite6_over_hermite_gpu": gpu_bat / gpu_4})
    elif kw:
        wall_32, gpu_32, _ = batched(systems, steps, energy, integrator)
        out.update({"batched_f32_hermite_wall_us_per_step": 1e6 * wall_32 / steps,
                    "batched_f32_hermite_gpu_us_per_step": 1e6 * gpu_32 / steps, "f64_over_f32_gpu": gpu_bat / gpu_32})
    elif integrator != "leapfrog":
        wall_lf, gpu_lf, _ = batched(systems, steps, energy, "leapfrog")
        out.update({"batched_leapfrog_wall_us_per_step": 1e6 * wall_lf / steps,
                    "batched_leapfrog_gpu_us_per_step": 1e6 * gpu_lf / steps,
                    "hermite_over_leapfrog_gpu": gpu_bat / gpu_lf})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sample", type=int, default=128)
    ap.add_argument("--cases", default="six,many,large")
    ap.add_argument("--integrator", choices=("leapfrog", "hermite", "hermite6", *BLOCK), default="leapfrog")
    ap.add_argument("--dtype", choices=("float32", "float64"), default="float32")
    ap.add_argument("--eta", type=float, default=0.02, help="the block integrators' accuracy parameter")
    ap.add_argument("--max-level", type=int, default=10, help="the block integrators' deepest level")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.dtype == "float64" and a.integrator == "leapfrog":
        ap.error("--dtype float64 needs --integrator hermite (there is no float64 leapfrog)")
    if a.integrator == "hermite6" or a.integrator in BLOCK:
        a.dtype = "float64"                               # the only number format of the 6th-order and the batched block schemes
    it, dt = a.integrator, getattr(torch, a.dtype)
    torch.cuda.set_device(0)
    out = {"device": torch.cuda.get_device_name(0)}
    todo = a.cases.split(",")
    bk = dict(eta=a.eta, max_level=a.max_level)
    if "six" in todo:
        out["six"] = case([3, 25, 50, 100, 250, 500], 1000, True, integrator=it, dtype=dt, block_kw=bk)
    if "many" in todo:
        out["many"] = case([100] * 1024, 100, True, sample=a.sample, integrator=it, dtype=dt, block_kw=bk)
    if "large" in todo:
        out["large"] = case([16384] * 4, 100, False, integrator=it, dtype=dt, block_kw=bk)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
