"""The rollout engine's pure parts (trainer.py, Trainer._rollout) and the models' shared decoder listing (gnn.py)
without a GPU: how the one host table of scenes laid side by side becomes the scenes' frames, and which Linears a
decoder holds."""
import numpy as np
import pandas as pd
import pytest
import torch

import contconv
import gnn
import trainer


def _frame_before_the_engine(filename, scene, table, times, sim_steps, n):
    """Trainer._rollout_frame as it stood when evaluate_rollout and evaluate_rollout_scenes each called it with one
    scene's own (steps, n, 18) table: the expectation is built from this, not from the code under test."""
    steps = np.repeat(np.arange(sim_steps), n)
    df_new = pd.DataFrame(table.reshape(sim_steps * n, 18), columns=trainer.ROLLOUT_COLUMNS[3:21])
    df_new.insert(0, "step", steps)
    df_new.insert(0, "scene", scene)
    df_new.insert(0, "filename", filename)
    df_new["step_time"] = np.repeat(times, n)
    return df_new[trainer.ROLLOUT_COLUMNS]


@pytest.mark.parametrize("sizes,scenes", [([3, 1, 4], [0, 1, 2]), ([5], [7])])
def test_scene_frames_split_the_table_scene_major(sizes, scenes):
    steps, n_all = 4, sum(sizes)
    rng = np.random.default_rng(5)
    # what the engine copies to the host: [ground truth | prediction] of all scenes' bodies, fp32 widened to float64
    table = rng.standard_normal((steps, n_all, 18)).astype(np.float32).astype(np.float64)
    times = rng.random(steps) / len(sizes)
    frames = trainer.Trainer._scene_frames("f.csv", scenes, sizes, table, times)
    assert len(frames) == len(sizes)
    lo = 0
    for frame, scene, n in zip(frames, scenes, sizes):
        own = np.ascontiguousarray(table[:, lo:lo + n])          # the scene's own table, as a per-scene rollout builds it
        want = _frame_before_the_engine("f.csv", scene, own, times, steps, n)
        pd.testing.assert_frame_equal(frame, want, check_exact=True)
        assert list(frame.columns) == trainer.ROLLOUT_COLUMNS and len(frame) == steps * n
        assert (frame["filename"] == "f.csv").all() and (frame["scene"] == scene).all()
        assert frame["step"].tolist() == [s for s in range(steps) for _ in range(n)]
        assert frame["step_time"].tolist() == [times[s] for s in range(steps) for _ in range(n)]
        # row (step s, body b) holds table[s, lo + b]
        assert np.array_equal(frame[trainer.ROLLOUT_COLUMNS[3:21]].to_numpy().reshape(steps, n, 18), table[:, lo:lo + n])
        lo += n
    # scene-major: all rows of scene 0, then all rows of scene 1, ...
    both = pd.concat(frames, ignore_index=True)
    assert both["scene"].tolist() == [sc for sc, n in zip(scenes, sizes) for _ in range(steps * n)]


def test_decoder_linears_of_a_linear_and_of_a_sequential():
    single = torch.nn.Linear(6, 3)
    assert gnn.decoder_linears(single) == [single]
    assert [(tuple(w.shape), act) for w, _, act in gnn.head_chain(single)] == [((3, 6), None)]
    lins = [torch.nn.Linear(6, 5), torch.nn.Linear(5, 4), torch.nn.Linear(4, 3)]
    seq = torch.nn.Sequential(lins[0], torch.nn.Tanh(), lins[1], torch.nn.Tanh(), lins[2])
    got = gnn.decoder_linears(seq)
    assert len(got) == 3 and all(a is b for a, b in zip(got, lins))
    chain = gnn.head_chain(seq)
    assert [act for _, _, act in chain] == ["tanh", "tanh", None]
    for (w, b, _), lin in zip(chain, lins):
        assert torch.equal(w, lin.weight) and torch.equal(b, lin.bias) and not w.requires_grad
    assert contconv.decoder_linears is gnn.decoder_linears      # one listing for both models


@pytest.mark.parametrize("hiddens", [None, [16, 8]])
def test_both_models_decoders_are_listed_alike(hiddens):
    g = gnn.GraphModel(input_dim=4, gnn_dim=8, message_passing_steps=1, output_hiddens=hiddens, device="cpu")
    c = contconv.ContinuousConvModel(continuous_conv_dim=8, decoder_hiddens=hiddens, device="cpu")
    for model in (g, c):
        lins = gnn.decoder_linears(model.output)
        assert len(lins) == 1 + len(hiddens or []) and lins[-1].out_features == 3
        assert [l.out_features for l in lins[:-1]] == (hiddens or [])
