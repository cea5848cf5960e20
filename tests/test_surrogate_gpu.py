"""HIP surrogate path (kNN / radius graph, EdgeConv GNN, ContinuousConv, Trainer.step / rollout)
against the CPU oracle (oracle/surrogate_oracle.py), through the C-ABI. Neighbour indices must be
BIT-EXACT; floating-point outputs within 1e-5 relative (north_star's bar), measured on the whole
tensor and per row (rows with a tiny reference norm are measured against the RMS row norm)."""
import numpy as np
import pytest
import torch

from conftest import global_rel, row_rel

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _plummer_pos(n, seed):
    from nbd.plummer import generate_plummer
    p, v, m = generate_plummer(n, seed=seed)
    return (torch.tensor(p, dtype=torch.float32), torch.tensor(v, dtype=torch.float32),
            torch.tensor(m, dtype=torch.float32))


def _batch(n, sizes):
    b = torch.cat([torch.full((s,), i, dtype=torch.int64) for i, s in enumerate(sizes)])
    assert b.numel() == n
    return b


# ------------------------------------------------------------------ graph build: index-exact
@pytest.mark.parametrize("n,k", [(1, 5), (2, 1), (10, 3), (10, 50), (65, 10), (200, 64), (500, 32), (500, 50),
                                 (300, 100), (400, 200), (4096, 32),
                                 (5000, 20), (8192, 8), (8193, 5)])      # staged form: second half of its lane words, its limit, past it
def test_knn_graph_bit_exact(n, k, gpu_device):
    from nbd import graphops
    from oracle import surrogate_oracle as so
    pos, _, _ = _plummer_pos(n, 10 + n)
    ref = so.knn_graph(pos, k)
    got = graphops.knn_graph(pos.cuda(), k).cpu()
    assert got.dtype == torch.int64 and got.shape == ref.shape
    assert torch.equal(got, ref)


def test_knn_graph_ties_and_loop(gpu_device):
    """Lattice points make exact distance ties: the lower index must win, as specified."""
    from nbd import graphops
    from oracle import surrogate_oracle as so
    g = torch.arange(6, dtype=torch.float32)
    pos = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).contiguous()    # 216 points
    for k, loop in ((6, False), (7, True), (26, False), (70, False)):
        assert torch.equal(graphops.knn_graph(pos.cuda(), k, loop=loop).cpu(), so.knn_graph(pos, k, loop=loop))


def test_knn_graph_batched(gpu_device):
    from nbd import graphops
    from oracle import surrogate_oracle as so
    pos, _, _ = _plummer_pos(300, 4)
    b = _batch(300, [100, 3, 1, 130, 66])
    for k in (2, 10, 70):
        assert torch.equal(graphops.knn_graph(pos.cuda(), k, batch=b.cuda()).cpu(), so.knn_graph(pos, k, batch=b))


@pytest.mark.parametrize("n,r,loop,cap", [(1, 1.0, True, 32), (50, 0.5, False, 32), (500, 1.0, True, 32),
                                          (500, 1.0, False, 32), (500, 0.3, True, 4), (2000, 1.0, True, 32),
                                          (300, 100.0, True, 7), (5000, 0.8, False, 32), (4097, 1.0, True, 3),
                                          (3000, 1.0, True, 4096)])       # last: cap too large for the streaming form
def test_radius_graph_bit_exact(n, r, loop, cap, gpu_device):
    from nbd import graphops
    from oracle import surrogate_oracle as so
    pos, _, _ = _plummer_pos(n, 20 + n)
    ref = so.radius_graph(pos, r, loop=loop, max_num_neighbors=cap)
    got = graphops.radius_graph(pos.cuda(), r, loop=loop, max_num_neighbors=cap).cpu()
    assert torch.equal(got, ref)
    # the transposed lists are the same edges sorted (stably) by edge_index[0]
    order = torch.sort(ref[0], stable=True).indices
    e = ref.shape[1]
    for scan in (False, True):      # O(E) scatter+sort transpose and the O(N^2) scanning one must agree
        lists = graphops.radius_lists(pos.cuda(), r, loop=loop, max_num_neighbors=cap, scan_transpose=scan)
        assert int(lists.rowptr[-1]) == e
        assert torch.equal(lists.centres[:e].cpu().to(torch.int64), ref[1][order])
        assert torch.equal(lists.rowptr.cpu().to(torch.int64)[1:], torch.cumsum(torch.bincount(ref[0], minlength=n), 0))


def test_radius_graph_batched(gpu_device):
    from nbd import graphops
    from oracle import surrogate_oracle as so
    pos, _, _ = _plummer_pos(400, 9)
    b = _batch(400, [150, 1, 249])
    ref = so.radius_graph(pos, 1.0, batch=b, loop=True, max_num_neighbors=16)
    assert torch.equal(graphops.radius_graph(pos.cuda(), 1.0, batch=b.cuda(), loop=True, max_num_neighbors=16).cpu(), ref)
    # many ragged graphs: segments straddle the 128-centre groups and the source slices of the streaming search
    pos, _, _ = _plummer_pos(3000, 10)
    b = _batch(3000, [3, 25, 50, 100, 250, 500, 1, 64, 128, 129, 700, 550, 500])
    for loop, cap in ((True, 32), (False, 5)):
        ref = so.radius_graph(pos, 0.9, batch=b, loop=loop, max_num_neighbors=cap)
        assert torch.equal(graphops.radius_graph(pos.cuda(), 0.9, batch=b.cuda(), loop=loop, max_num_neighbors=cap).cpu(), ref)


def test_radius_graph_without_self_loops_searches_cap_plus_one_then_drops_self(gpu_device):
    """torch_cluster 1.6.3 (contconv.py:225 with self_loops=False): radius(x, x, r, max_num_neighbors + 1) with self as
    a candidate, then row == col dropped. A centre with >= 33 lower-indexed hits never meets itself and returns 33."""
    from nbd import graphops
    from oracle import surrogate_oracle as so
    g = torch.Generator().manual_seed(5)
    pos = torch.rand(80, 3, generator=g) * 0.2                     # everything within r = 1 of everything
    ref = so.radius_graph(pos, 1.0, loop=False, max_num_neighbors=32)
    deg = torch.bincount(ref[1], minlength=80)
    assert deg[:33].eq(32).all() and deg[33:].eq(33).all()          # centres 33.. have >= 33 lower-indexed hits
    for cache in (None, graphops.RadiusCache()):
        lists = graphops.radius_lists(pos.cuda(), 1.0, loop=False, max_num_neighbors=32, cache=cache)
        assert torch.equal(lists.deg.cpu().to(torch.int64), deg)
        e = ref.shape[1]
        order = torch.sort(ref[0], stable=True).indices
        assert int(lists.rowptr[-1]) == e
        assert torch.equal(lists.centres[:e].cpu().to(torch.int64), ref[1][order])
    assert torch.equal(graphops.radius_graph(pos.cuda(), 1.0, loop=False, max_num_neighbors=32).cpu(), ref)
    # a clump inside a larger system, both loop modes, odd caps
    pos2, _, _ = _plummer_pos(700, 77)
    pos2[100:180] = pos2[100] + (torch.rand(80, 3, generator=g) - 0.5) * 0.05
    for loop, cap in ((False, 32), (False, 5), (True, 32)):
        assert torch.equal(graphops.radius_graph(pos2.cuda(), 0.6, loop=loop, max_num_neighbors=cap).cpu(),
                           so.radius_graph(pos2, 0.6, loop=loop, max_num_neighbors=cap))


def test_radius_squared_is_the_double_product_cast_to_fp32(gpu_device):
    """r = 0.7: float(0.7 * 0.7) = 0.49000001 is one ulp above fp32(0.7)^2 = 0.48999998. A body at distance exactly
    fp32(0.7) (d2 = 0.48999998) is a neighbour under torch_cluster's rule and was not under the fp32 product."""
    from nbd import graphops
    from oracle import surrogate_oracle as so
    x = float(np.float32(0.7))
    assert np.float32(x) * np.float32(x) < np.float32(0.7 * 0.7)
    pos = torch.tensor([[0., 0, 0], [x, 0, 0], [0, 5, 0], [0, 5 + x, 0], [9, 9, 9]])
    ref = so.radius_graph(pos, 0.7, loop=False)
    assert ref.tolist() == [[1, 0, 3, 2], [0, 1, 2, 3]]
    assert torch.equal(graphops.radius_graph(pos.cuda(), 0.7, loop=False).cpu(), ref)
    assert graphops.radius_r2(0.7) == float(np.float32(0.7 * 0.7)) == so.radius_r2(0.7)
    lists = graphops.radius_lists(pos.cuda(), 0.7, loop=True)
    assert lists.deg.cpu().tolist() == [2, 2, 2, 2, 1]


def test_knn_graph_with_coincident_bodies(gpu_device):
    """torch_cluster 1.6.3: knn(x, x, k + 1) with self as a candidate, then row == col dropped. With coincident bodies
    the ties go to the lower index; a centre with >= k + 1 lower-indexed bodies at distance 0 keeps k + 1 neighbours."""
    from nbd import graphops
    from oracle import surrogate_oracle as so
    pos, _, _ = _plummer_pos(300, 31)
    pos[40:46] = pos[40]                     # six coincident bodies
    pos[200] = pos[7]; pos[250] = pos[7]     # and a triple far apart in index
    for k in (1, 2, 5, 10, 50):
        ref = so.knn_graph(pos, k)
        got = graphops.knn_graph(pos.cuda(), k).cpu()
        assert torch.equal(got, ref), k
        if k >= 5:                           # no centre has k + 1 coincident lower-indexed bodies: regular degree
            assert ref.shape[1] == 300 * k
            # ... and then the rollout's fast path (diagonal masked in the kernel, hint / out buffers) is the same graph
            buf = graphops.knn_graph(pos.cuda(), k, loop=False, hint=got.cuda(), out=got.cuda().clone())
            assert torch.equal(buf.cpu(), ref)
    ref1 = so.knn_graph(pos, 1)
    assert ref1.shape[1] > 300                          # the corner really occurs at k = 1 (bodies 42-45, 250)
    # The ONE documented divergence: the rollout's fast path (out= / hint= / inside a capture) masks the diagonal
    # in the kernel and always returns k neighbours per centre, where the k + 1-then-drop-self rule keeps k + 1 for a centre
    # with >= k + 1 lower-indexed bodies at distance exactly 0. Every edge of the fast path is one of the rule's, centres
    # outside that corner get exactly the same neighbours, and the corner's centres lose their LAST (highest-index) one.
    fast = graphops.knn_graph(pos.cuda(), 1, loop=False, out=torch.empty((2, 300), dtype=torch.int64, device="cuda")).cpu()
    assert fast.shape == (2, 300) and torch.equal(fast[1], torch.arange(300))
    ref_edges = {(int(a), int(b)) for a, b in ref1.t().tolist()}
    assert all((int(a), int(b)) in ref_edges for a, b in fast.t().tolist())
    deg = torch.bincount(ref1[1], minlength=300)
    corner = set(torch.nonzero(deg == 2).flatten().tolist())
    assert corner == {42, 43, 44, 45, 250}
    for c in range(300):
        mine = sorted(int(a) for a, b in ref1.t().tolist() if int(b) == c)
        assert int(fast[0, c]) == mine[0], c           # the first (lowest-index among ties) neighbour either way
    b = _batch(300, [60, 140, 100])
    for k in (2, 7):
        assert torch.equal(graphops.knn_graph(pos.cuda(), k, batch=b.cuda()).cpu(), so.knn_graph(pos, k, batch=b))


# ------------------------------------------------------------------ dense blocks
@pytest.mark.parametrize("n,k,m", [(1, 4, 3), (100, 4, 128), (4096, 8, 64), (333, 7, 5), (1000, 68, 3), (257, 64, 64),
                                   (700, 128, 128), (129, 1000, 130), (64, 256, 32),
                                   (1000, 2048, 128), (700, 1028, 200), (513, 512, 96)])   # last three: split-K 128x128 path
def test_linear_matches_torch(n, k, m, gpu_device):
    from nbd import nnops
    g = torch.Generator().manual_seed(n * 7 + k)
    x, w, b = torch.randn(n, k, generator=g), torch.randn(m, k, generator=g) / k ** 0.5, torch.randn(m, generator=g)
    ref = x.double() @ w.double().t() + b.double()
    got = nnops.linear(x.cuda(), w.cuda(), b.cuda()).cpu()
    assert global_rel(got, ref) < 2e-6
    got_t = nnops.linear(x.cuda(), w.cuda(), b.cuda(), act="tanh").cpu()
    assert (got_t.double() - torch.tanh(ref)).abs().max() < 5e-6
    # no bias, row scale, bias row scale, strided output slice
    rs, brs = torch.rand(n, generator=g) + 0.5, torch.rand(n, generator=g)
    wide = torch.zeros(n, m + 5).cuda()
    nnops.linear(x.cuda(), w.cuda(), b.cuda(), out=wide[:, 5:], rowscale=rs.cuda(), bias_rowscale=brs.cuda())
    ref2 = rs.double()[:, None] * (x.double() @ w.double().t()) + brs.double()[:, None] * b.double()
    assert global_rel(wide[:, 5:].cpu(), ref2) < 2e-6 and (wide[:, :5] == 0).all()


def test_linear_asymmetric_operands(gpu_device):
    """A = I against an asymmetric W catches a transposed fragment map (MFMA C/D layout)."""
    from nbd import nnops
    w = torch.arange(96 * 64, dtype=torch.float32).reshape(96, 64)
    out = nnops.linear(torch.eye(64).cuda(), w.cuda()).cpu()
    assert torch.equal(out, w.t())


def test_layernorm_matches_torch(gpu_device):
    from nbd import nnops
    for n, c in ((5, 68), (1000, 256), (77, 4), (300, 130)):
        x = torch.randn(n, c) * 3 + 1
        ln = torch.nn.LayerNorm(c)
        with torch.no_grad():
            ln.weight.uniform_(0.5, 1.5); ln.bias.uniform_(-1, 1)
            ref = ln(x)
        got = nnops.layernorm(x.cuda(), ln.weight.detach().cuda(), ln.bias.detach().cuda(), ln.eps).cpu()
        assert (got - ref).abs().max() < 5e-6


@pytest.mark.parametrize("n,dims", [(1000, [256, 64, 32, 3]), (77, [130, 20, 3]), (5, [68, 3]), (300, [4, 7, 64, 8]),
                                    (2, [256, 64, 64, 1]), (513, [200, 33, 5])])
def test_layernorm_decoder_in_one_launch_matches_torch(n, dims, gpu_device):
    """nbd_ln_mlp_head_f32 (LayerNorm + tanh MLP decoder + optional half-kick) against torch fp64, and against the
    separate launches it replaces; shapes outside it report themselves (plan None)."""
    from gnn import head_chain, run_chain
    from nbd import nnops
    torch.manual_seed(len(dims) * 1000 + n)
    c = dims[0]
    x = torch.randn(n, c) * 2 + 0.5
    ln = torch.nn.LayerNorm(c)
    layers = []
    for i in range(len(dims) - 1):
        layers.append(torch.nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            layers.append(torch.nn.Tanh())
    mlp = torch.nn.Sequential(*layers) if len(layers) > 1 else layers[0]
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5); ln.bias.uniform_(-1, 1)
        ref = mlp.double()(ln.double()(x.double())).float()
    mlp, ln = mlp.float().cuda(), ln.float().cuda()
    head = head_chain(mlp)
    plan = nnops.ln_mlp_head_plan(c, head, ln.weight.detach(), ln.bias.detach())
    assert plan is not None
    xg = x.cuda()
    got = nnops.ln_mlp_head(xg, ln.weight.detach(), ln.bias.detach(), ln.eps, plan)
    assert (got.cpu() - ref).abs().max() < 1e-5 * max(1.0, float(ref.abs().max()))
    sep = run_chain(nnops.layernorm(xg, ln.weight.detach(), ln.bias.detach(), ln.eps), head)
    assert (got - sep).abs().max() < 1e-5 * max(1.0, float(ref.abs().max()))
    # a column slice of a wider buffer as input, the caller's buffer as output, the half-kick in the epilogue
    wide = torch.randn(n, c + 5, device="cuda")
    wide[:, 2:2 + c] = xg
    vel = torch.randn(n, dims[-1], device="cuda")
    v0 = vel.clone()
    out = torch.empty(n, dims[-1], device="cuda")
    got2 = nnops.ln_mlp_head(wide[:, 2:2 + c], ln.weight.detach(), ln.bias.detach(), ln.eps, plan, out=out, kick_vel=vel, kick_c=0.25)
    assert got2.data_ptr() == out.data_ptr() and torch.equal(got2, got)
    assert torch.equal(vel, v0 + 0.25 * got)
    # outside the kernel's shapes: no plan
    assert nnops.ln_mlp_head_plan(300, [(torch.zeros(3, 300), None, None)]) is None
    assert nnops.ln_mlp_head_plan(64, [(torch.zeros(100, 64), None, "tanh"), (torch.zeros(3, 100), None, None)]) is None


def _copy_state(dst, src):
    missing = dst.load_state_dict(src.state_dict(), strict=True)
    return missing


# ------------------------------------------------------------------ GNN
@pytest.mark.parametrize("cfg", [
    dict(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", neighbors=10),            # published (gnn_experiment.py:61-72)
    dict(input_dim=4, gnn_dim=32, message_passing_steps=3, aggr="sum", neighbors=5, output_hiddens=[16, 8]),
    dict(input_dim=7, gnn_dim=48, message_passing_steps=1, aggr="mean", neighbors=8, node_encoder_dims=[20, 24]),
    dict(input_dim=7, gnn_dim=128, message_passing_steps=2, aggr="sum", neighbors=6),       # H = 128: general path only
    dict(input_dim=4, gnn_dim=100, message_passing_steps=1, aggr="mean", neighbors=70, output_dim=5),
    dict(input_dim=4, gnn_dim=40, message_passing_steps=2, aggr="max", neighbors=9),          # PyG EdgeConv's own default
    # H = 64 beyond the published shape (the MFMA-tail kernel's other epilogues and inputs): 7 features formed on the fly,
    # three layers (a folded next-[P|Q] fed from [P|Q]), sum aggregation, LayerNorm handed to an MLP head ...
    dict(input_dim=7, gnn_dim=64, message_passing_steps=3, aggr="sum", neighbors=6, output_hiddens=[16]),
    # ... and behind an encoder: 64 encoder columns, the first [P|Q] from a Linear, LayerNorm over 128
    dict(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", neighbors=7, node_encoder_dims=[24]),
])
def test_gnn_forward_matches_oracle(cfg, gpu_device):
    import gnn
    from nbd.data import Data
    from oracle import surrogate_oracle as so
    torch.manual_seed(1)
    ocfg = {k: v for k, v in cfg.items()}
    ora = so.GraphModelOracle(**ocfg).eval()
    model = gnn.GraphModel(device="cuda", **cfg)
    _copy_state(model, ora)
    pos, vel, m = _plummer_pos(700, 5)
    x7 = torch.cat([pos, vel, m[:, None] * 700], 1)
    ei = so.knn_graph(pos, cfg["neighbors"])
    with torch.no_grad():
        ref = ora.forward_graph(x7, ei)
    for fused in (True, False):                 # one-launch-per-layer kernel and the general path
        model.use_fused = fused
        got = model.predict_graph(Data(x=x7.cuda(), edge_index=ei.cuda())).cpu()
        assert global_rel(got, ref) < TOL and row_rel(got, ref) < 10 * TOL, fused
        d = Data(x=x7.cuda(), edge_index=ei.cuda()); d._regular_k = cfg["neighbors"]
        assert global_rel(model.predict_graph(d).cpu(), ref) < TOL, fused
    model.use_fused = True
    # ragged graph (arbitrary edge order, a node without edges): general CSR path
    keep = torch.rand(ei.shape[1], generator=torch.Generator().manual_seed(3)) < 0.7
    keep &= ei[1] != 13
    ei2 = ei[:, keep][:, torch.randperm(int(keep.sum()), generator=torch.Generator().manual_seed(4))]
    with torch.no_grad():
        ref2 = ora.forward_graph(x7, ei2)
    for fused in (True, False):
        model.use_fused = fused
        got2 = model.predict_graph(Data(x=x7.cuda(), edge_index=ei2.cuda())).cpu()
        assert global_rel(got2, ref2) < TOL, fused


def test_gnn_predict_uses_k50_like_reference(gpu_device):
    import gnn
    from oracle import surrogate_oracle as so
    torch.manual_seed(2)
    ora = so.GraphModelOracle(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", neighbors=10).eval()
    model = gnn.GraphModel(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", neighbors=10, device="cuda")
    _copy_state(model, ora)
    pos, vel, m = _plummer_pos(512, 6)
    feat = torch.cat([vel, m[:, None] * 512], 1)
    ref = ora.predict(pos, feat, k=50)
    got = model.predict(pos.cuda(), feat.cuda()).cpu()
    assert global_rel(got, ref) < TOL
    assert global_rel(model.predict(pos.cuda(), feat.cuda(), neighbors=32).cpu(), ora.predict(pos, feat, k=32)) < TOL
    data = gnn.transform_to_graph(pos.cuda(), feat.cuda(), torch.zeros(512, 3).cuda())
    assert data.edge_index.shape == (2, 512 * 50) and data.x.shape == (512, 7)
    assert model.neighbors == 10 and model.get_config()["gnn_dim"] == 64


# ------------------------------------------------------------------ ContinuousConv
@pytest.mark.parametrize("agg,D,I,O", [("mean", 4, 8, 16), ("sum", 6, 4, 8), ("mean", 3, 70, 40),
                                       ("mean", 4, 32, 128), ("sum", 3, 64, 96), ("mean", 5, 128, 130), ("mean", 2, 96, 20)])
def test_contconv_layer_matches_oracle(agg, D, I, O, gpu_device):
    """One ContinuousConv layer vs the oracle, which calls F.grid_sample exactly as contconv.py:73-75."""
    import contconv
    from oracle import surrogate_oracle as so
    torch.manual_seed(D)
    pos, _, _ = _plummer_pos(400, 8)
    feat = torch.randn(400, I)
    ora = so.ContinuousConvOracle(I, O, D, radius=1.0, agg=agg)
    layer = contconv.ContinuousConv(I, O, D, radius=1.0, agg=agg).cuda()
    _copy_state(layer, ora)
    ei = so.radius_graph(pos, 1.0, loop=True, max_num_neighbors=32)
    with torch.no_grad():
        ref = ora(pos, feat, ei)
        got = layer(pos.cuda(), feat.cuda(), edge_index=ei.cuda()).cpu()
        assert global_rel(got, ref) < TOL and row_rel(got, ref) < 10 * TOL
        # uncapped dense graph: in-degree up to 150, many pairs per (node, filter cell)
        ei_d = so.radius_graph(pos[:150], 3.0, loop=True, max_num_neighbors=150)
        ref_d = ora(pos[:150], feat[:150], ei_d)
        got_d = layer(pos[:150].cuda(), feat[:150].contiguous().cuda(), edge_index=ei_d.cuda()).cpu()
        assert global_rel(got_d, ref_d) < TOL


@pytest.mark.parametrize("n,D,I,O,agg,r,cap", [
    (400, 4, 8, 16, "mean", 1.0, 32), (1000, 6, 128, 128, "mean", 1.0, 32), (129, 3, 4, 20, "sum", 1.0, 32),
    (513, 5, 96, 130, "mean", 0.8, 32), (300, 4, 32, 64, "sum", 3.0, 300), (64, 2, 12, 33, "mean", 1.0, 32),
    (2000, 6, 64, 96, "mean", 0.6, 32), (1, 4, 8, 8, "mean", 1.0, 32),
    (300, 5, 7, 33, "mean", 1.0, 32), (350, 3, 70, 40, "sum", 1.0, 32), (200, 4, 1, 5, "mean", 1.0, 32)])   # in_channels % 4 != 0: padded columns
def test_contconv_fused_kernels_match_oracle_and_binned_path(n, D, I, O, agg, r, cap, gpu_device):
    """csrc/contconv_fused.hip (pair lists + gather/MFMA/accumulate in one kernel) against the oracle and against
    the round-1 formulation (dense binned matrix + GEMM) on the same edges: ragged tile counts, nodes without
    edges, rows with hundreds of pairs (r = 3, uncapped), channel counts off the MFMA grid, both aggregations."""
    import contconv
    from oracle import surrogate_oracle as so
    torch.manual_seed(n + D)
    pos, _, _ = _plummer_pos(n, 30 + D)
    feat = torch.randn(n, I)
    ora = so.ContinuousConvOracle(I, O, D, radius=r, agg=agg)
    layer = contconv.ContinuousConv(I, O, D, radius=r, agg=agg).cuda()
    _copy_state(layer, ora)
    assert layer.fused_ok()
    ei = so.radius_graph(pos, r, loop=True, max_num_neighbors=cap)
    with torch.no_grad():
        ref = ora(pos, feat, ei)
        got = layer(pos.cuda(), feat.cuda(), edge_index=ei.cuda())
        again = layer(pos.cuda(), feat.cuda(), edge_index=ei.cuda())
        assert torch.equal(got, again)                                      # deterministic
        layer.use_fused = False
        old = layer(pos.cuda(), feat.cuda(), edge_index=ei.cuda())
        layer.use_fused = True
        got_t = layer(pos.cuda(), feat.cuda(), edge_index=ei.cuda(), act="tanh")
    assert global_rel(got.cpu(), ref) < TOL and row_rel(got.cpu(), ref) < 10 * TOL
    assert global_rel(got.cpu(), old.cpu()) < TOL
    assert global_rel(got_t.cpu(), torch.tanh(ref)) < TOL
    # a strided output / input view (how the model passes its concatenation buffer)
    buf = torch.zeros((n, I + O + 2), device="cuda")
    buf[:, :I] = feat.cuda()
    with torch.no_grad():
        layer(pos.cuda(), buf[:, :I], edge_index=ei.cuda(), out=buf[:, I:I + O]) if (I + O + 2) % 2 == 0 else None
    if (I + O + 2) % 2 == 0:
        assert torch.equal(buf[:, I:I + O], got) and float(buf[:, I + O:].abs().max()) == 0.0


@pytest.mark.parametrize("agg", ["max", "min"])
@pytest.mark.parametrize("D,I,O", [(4, 8, 16), (3, 70, 40)])
def test_contconv_extreme_aggregations_match_oracle(agg, D, I, O, gpu_device):
    """scatter(reduce="max"/"min") (contconv.py:95-97 passes `agg` straight through): per-edge messages
    materialised through the virtual one-edge-per-row graph, then the segment reduction; rows without edges 0.
    (I = 70: not a multiple of 4 -- the fused kernel runs on zero-padded feature columns.)"""
    import contconv
    from oracle import surrogate_oracle as so
    torch.manual_seed(D)
    pos, _, _ = _plummer_pos(300, 9)
    feat = torch.randn(300, I)
    ora = so.ContinuousConvOracle(I, O, D, radius=1.0, agg=agg)
    layer = contconv.ContinuousConv(I, O, D, radius=1.0, agg=agg).cuda()
    _copy_state(layer, ora)
    ei = so.radius_graph(pos, 1.0, loop=False, max_num_neighbors=32)          # no self loops: isolated nodes exist
    assert (torch.bincount(ei[0], minlength=300) == 0).any()
    with torch.no_grad():
        ref = ora(pos, feat, ei)
        got = layer(pos.cuda(), feat.cuda(), edge_index=ei.cuda()).cpu()
    assert global_rel(got, ref) < TOL and row_rel(got, ref) < 10 * TOL
    assert float(got[torch.bincount(ei[0], minlength=300) == 0].abs().max()) == 0.0
    with pytest.raises(NotImplementedError):
        contconv.ContinuousConv(I, O, D, agg="median")              # not one of torch_scatter's reductions
    # (training through max / min: tests/test_train_gpu.py::test_contconv_extreme_aggregations_train; "mul": below)


@pytest.mark.parametrize("D,I,O", [(4, 8, 16), (3, 70, 40)])
def test_contconv_product_aggregation_matches_oracle_and_trains(D, I, O, gpu_device):
    """scatter(reduce="mul") (contconv.py:95-97 passes `agg` straight through; torch_scatter's scatter_mul starts from
    ones): the product of a row's messages, 1 for a row without any, forward and backward (each message's gradient is the
    product of the others -- prefix times suffix, exact with zero messages) against autograd on the oracle. The bar is
    TOL per factor: a product of up to `cap` messages carries the sum of their relative errors, so cap = 4 here."""
    import contconv
    from oracle import surrogate_oracle as so
    cap = 4
    torch.manual_seed(D + 40)
    n = 200
    pos, _, _ = _plummer_pos(n, 9)
    feat = torch.randn(n, I)
    dout = torch.randn(n, O)
    ora = so.ContinuousConvOracle(I, O, D, radius=1.0, agg="mul")
    layer = contconv.ContinuousConv(I, O, D, radius=1.0, agg="mul").cuda()
    _copy_state(layer, ora)
    ei = so.radius_graph(pos, 1.0, loop=False, max_num_neighbors=cap)
    lonely = torch.bincount(ei[0], minlength=n) == 0
    assert lonely.any()
    with torch.no_grad():
        ref = ora(pos, feat, ei)
        got = layer(pos.cuda(), feat.cuda(), edge_index=ei.cuda()).cpu()
    assert global_rel(got, ref) < cap * TOL
    assert torch.equal(got[lonely], torch.ones_like(got[lonely]))
    fr = feat.clone().requires_grad_()
    torch.tanh(ora(pos, fr, ei)).backward(dout)
    fg = feat.clone().cuda().requires_grad_()
    out = layer(pos.cuda(), fg, edge_index=ei.cuda(), act="tanh")
    out.backward(dout.cuda())
    assert global_rel(fg.grad.cpu(), fr.grad) < cap * TOL
    assert global_rel(layer.filters.grad.cpu(), ora.filters.grad) < cap * TOL
    # a zero message: the other rows' gradients vanish, its own is the product of the others (no division anywhere)
    from nbd import nnops
    m = torch.tensor([[2.0, 0.0], [3.0, 5.0], [4.0, 0.0], [7.0, 7.0]], device="cuda")
    rowptr = torch.tensor([0, 3, 3, 4], dtype=torch.int32, device="cuda")
    x = nnops.segment_reduce(m, rowptr, 3, "mul")
    assert torch.equal(x.cpu(), torch.tensor([[24.0, 0.0], [1.0, 1.0], [7.0, 7.0]]))
    dm = nnops.segment_mul_bwd(m, rowptr, 3, torch.ones((3, 2), device="cuda"))
    assert torch.equal(dm.cpu(), torch.tensor([[12.0, 0.0], [8.0, 0.0], [6.0, 0.0], [1.0, 1.0]]))


def test_gnn_predict_through_one_cabi_call_equals_the_per_kernel_path(gpu_device):
    """predict() enqueues the kNN search and the fused layers through nbd_gnn_forward_f32 (one ctypes call) from its
    second call on: same graph, and -- without the exponential tables -- same kernels, same bits as the per-kernel
    calls, over a drifting sequence. With the tables (the default: tanh(P + Q) as 1 - 2 / (2^(cP) 2^(cQ) + 1), the
    first layer's rows written by the search kernel) the graph is still identical and the output within the 1e-5 bar."""
    import gnn
    torch.manual_seed(4)
    pos, vel, m = _plummer_pos(700, 12)
    pos, vel, m1 = pos.cuda(), vel.cuda(), (m * 700)[:, None].cuda()
    a = gnn.GraphModel(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", device="cuda")
    b = gnn.GraphModel(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", device="cuda")
    t = gnn.GraphModel(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", device="cuda")
    b.load_state_dict(a.state_dict())
    t.load_state_dict(a.state_dict())
    a.use_exp_tables = False
    b.use_one_call = False
    for step in range(5):
        feat = torch.cat([vel, m1], 1)
        ya, yb, yt = a.predict(pos, feat), b.predict(pos, feat), t.predict(pos, feat)
        assert torch.equal(ya, yb), step
        assert torch.equal(a._knn_buf, b._knn_buf) and torch.equal(t._knn_buf, b._knn_buf)
        assert (yt - yb).abs().max() <= TOL * max(1.0, float(yb.abs().max())), step
        if step:
            assert a._one_call is not None and b._one_call is None
            assert t._one_call["fa"].workspace_bytes > 0 and a._one_call["fa"].workspace_bytes == 0
        pos = pos + 0.01 * vel
    # k override and a changed n re-plan instead of reusing stale pointers
    for mdl in (a, t):
        for _ in range(2):
            got = mdl.predict(pos[:300].contiguous(), feat[:300].contiguous(), neighbors=7)
            ref = b.predict(pos[:300].contiguous(), feat[:300].contiguous(), neighbors=7)
            assert torch.equal(got, ref) if mdl is a else (got - ref).abs().max() <= TOL * max(1.0, float(ref.abs().max()))


def test_gnn_exponential_tables_survive_preactivations_out_of_their_range(gpu_device):
    """An entry of the tables whose |2 log2(e) v| exceeds 100 holds NaN, and a node that meets one is recomputed from
    P / Q exactly as without tables: scaled-up first-layer weights (pre-activations in the hundreds, opposite signs
    cancelling inside tanh) must give the per-kernel path's result."""
    import gnn
    torch.manual_seed(9)
    pos, vel, m = _plummer_pos(600, 5)
    pos, vel, m1 = pos.cuda(), vel.cuda(), (m * 600)[:, None].cuda()
    t = gnn.GraphModel(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", device="cuda")
    with torch.no_grad():
        for p in t.gnns[0].parameters():            # first EdgeConv: both Linears of its message MLP
            p.mul_(60.0)
    b = gnn.GraphModel(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", device="cuda")
    b.load_state_dict(t.state_dict())
    b.use_one_call = False
    feat = torch.cat([vel * 30.0, m1], 1)
    for step in range(3):
        yt, yb = t.predict(pos, feat), b.predict(pos, feat)
        assert torch.isfinite(yt).all()
        assert (yt - yb).abs().max() <= TOL * max(1.0, float(yb.abs().max())), step
    assert t._one_call is not None and t._one_call["fa"].workspace_bytes > 0


@pytest.mark.parametrize("scale", [4.0, 12.0, 25.0])
def test_gnn_exponential_tables_hold_the_bar_for_large_preactivations_inside_their_range(scale, gpu_device):
    """tanh(P_i + Q_j) through the tables loses accuracy as |P| and |Q| grow inside the accepted range (the rounding of
    2 log2(e) v is magnified where P + Q is near 0; csrc/gnn_fused.hip states the bound: 4e-6 absolute at the limit). Models
    whose first-layer weights are scaled up -- pre-activations from a few units to the limit of the range and past it -- must
    still meet the oracle at 1e-5, through the one-call pass with tables (advisor, round 3)."""
    import gnn
    from oracle import surrogate_oracle as so
    torch.manual_seed(int(scale))
    cfg = dict(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", neighbors=10)
    ora = so.GraphModelOracle(**cfg).eval()
    with torch.no_grad():
        lin = ora.gnns[0].nn[0]                       # P = W[:, :F] x_i - W[:, F:] x_i, Q = W[:, F:] x_j: both grow with the scale
        lin.weight.mul_(scale)
    model = gnn.GraphModel(device="cuda", **cfg)
    _copy_state(model, ora)
    n = 1500
    pos, vel, m = _plummer_pos(n, 77)
    feat = torch.cat([vel, m[:, None] * n], 1)
    ref = ora.predict(pos, feat, k=50)
    got = model.predict(pos.cuda(), feat.cuda()).cpu()
    assert model.last_path == "one_call+tables"
    assert global_rel(got, ref) < TOL and row_rel(got, ref) < 10 * TOL, scale
    # the pre-activations really are large: 2 log2(e) |Q| of the first layer reaches tens at these scales
    x = torch.cat([pos, m[:, None] * n], 1)
    q = (x @ lin.weight[:, 4:].t()).abs().max().item() * 2.8853900817779268
    assert q > 10.0 * scale / 4.0


def test_contconv_fused_refuses_a_row_beyond_its_16_bit_counters_loudly(gpu_device):
    """The pair kernel counts pairs per (node, cell) in 16 bits: a node with more than 65 535 edges cannot be binned.
    Its tile is refused -- NaN for the tile's 128 nodes -- and every other tile is computed as usual."""
    import contconv
    n = 70000
    g = torch.Generator().manual_seed(3)
    pos = torch.rand(n, 3, generator=g) * 0.3
    feat = torch.randn(n, 4, generator=g)
    hub_src = torch.arange(1, 66001)
    row = torch.cat([torch.zeros(66000, dtype=torch.int64), torch.arange(200, 400)])       # node 0: 66 000 edges
    col = torch.cat([hub_src, torch.arange(5000, 5200)])
    ei = torch.stack([row, col]).cuda()
    layer = contconv.ContinuousConv(4, 8, 4, radius=1.0, agg="sum").cuda()
    with torch.no_grad():
        out = layer(pos.cuda(), feat.cuda(), edge_index=ei).cpu()
        ok = layer(pos.cuda(), feat.cuda(), edge_index=ei[:, 66000:]).cpu()
    assert torch.isnan(out[:128]).all()
    assert torch.isfinite(out[128:]).all() and torch.equal(out[128:], ok[128:])


def test_contconv_model_matches_oracle(gpu_device):
    import contconv
    from oracle import surrogate_oracle as so
    torch.manual_seed(3)
    cfg = dict(in_channels=4, out_channels=3, filter_resolution=[4, 3], radius=1.0, agg="mean", self_loops=True,
               continuous_conv_layers=2, continuous_conv_dim=16, encoder_hiddens=[8, 12], decoder_hiddens=[10, 6])
    ora = so.ContinuousConvModelOracle(**cfg)
    with torch.no_grad():                       # non-trivial BatchNorm running statistics
        for nrm in ora.node_encoder.norms:
            nrm.module.running_mean.uniform_(-0.5, 0.5); nrm.module.running_var.uniform_(0.5, 2.0)
            nrm.module.weight.uniform_(0.5, 1.5); nrm.module.bias.uniform_(-0.3, 0.3)
    ora.eval()
    model = contconv.ContinuousConvModel(device="cuda", **cfg)
    _copy_state(model, ora)
    pos, vel, m = _plummer_pos(600, 12)
    feat = torch.cat([vel, m[:, None] * 600], 1)
    ref = ora.predict(pos, feat)
    got = model.predict(pos.cuda(), feat.cuda()).cpu()
    assert global_rel(got, ref) < TOL and row_rel(got, ref) < 10 * TOL
    assert model.neighbors == 0
    # no encoder / no self loops / sum aggregation / single Linear head
    cfg2 = dict(in_channels=4, out_channels=3, filter_resolution=[5], radius=0.7, agg="sum", self_loops=False,
                continuous_conv_layers=1, continuous_conv_dim=24)
    ora2 = so.ContinuousConvModelOracle(**cfg2).eval()
    model2 = contconv.ContinuousConvModel(device="cuda", **cfg2)
    _copy_state(model2, ora2)
    assert global_rel(model2.predict(pos.cuda(), feat.cuda()).cpu(), ora2.predict(pos, feat)) < TOL
    with pytest.raises(AttributeError):
        contconv.ContinuousConvModel(filter_resolution=4)
    # a batch of three graphs (eval_graph_batch path: radius search restricted to batch segments)
    from nbd.data import Data
    b = _batch(600, [250, 1, 349])
    x7 = torch.cat([pos, feat], 1)
    with torch.no_grad():
        ref_b = ora.forward_x(x7, batch=b)
    got_b = model.forward(Data(x=x7.cuda(), batch=b.cuda()))     # outside no_grad: the autograd path
    assert got_b.requires_grad
    got_b = got_b.detach().cpu()
    assert global_rel(got_b, ref_b) < TOL
    y = torch.randn(600, 3)
    rmse, mse, secs = model.eval_graph_batch(Data(x=x7.cuda(), batch=b.cuda(), y=y.cuda()))
    assert mse == pytest.approx(torch.nn.functional.mse_loss(ref_b, y).item(), rel=1e-4) and rmse == pytest.approx(mse ** 0.5, rel=1e-5) and secs > 0


# ------------------------------------------------------------------ Trainer
def test_trainer_step_and_rollout(gpu_device):
    import gnn
    import trainer
    from nbd.data import Data
    from oracle import surrogate_oracle as so
    torch.manual_seed(4)
    ora = so.GraphModelOracle(input_dim=4, gnn_dim=32, message_passing_steps=2, aggr="mean", neighbors=10).eval()
    model = gnn.GraphModel(input_dim=4, gnn_dim=32, message_passing_steps=2, aggr="mean", neighbors=10, device="cuda")
    _copy_state(model, ora)
    tr = trainer.Trainer(model, optimizer=None, device="cuda", dt=0.01)
    n, steps, dt = 128, 4, 0.01
    pos, vel, m = _plummer_pos(n, 2)
    m1 = (m * n)[:, None]
    acc = ora.predict(pos, torch.cat([vel, m1], 1))
    # one Trainer.step (trainer.py:217-226) vs the oracle restatement
    p_ref, v_ref, a_ref = so.trainer_step(lambda p, f: ora.predict(p, f), pos, vel, m1, acc, dt)
    p_got, v_got, a_got = tr.step(pos.cuda(), vel.cuda(), m1.cuda(), acc.cuda(), dt)
    assert torch.equal(p_got.cpu(), p_ref)                     # kick/drift are bit-exact given the same acc
    assert global_rel(a_got.cpu(), a_ref) < TOL and global_rel(v_got.cpu(), v_ref) < TOL
    # evaluate_rollout: ground truth = the oracle rollout itself -> errors ~ fp32 noise, schema as reference
    xs, ys, st = [], [], []
    p, v, a = pos, vel, acc
    for s in range(steps):
        xs.append(torch.cat([p, v, m1], 1)); ys.append(a); st.append(torch.full((n,), s))
        p, v, a = so.trainer_step(lambda pp, ff: ora.predict(pp, ff), p, v, m1, a, dt)
    data = Data(x=torch.cat(xs), y=torch.cat(ys), step=torch.cat(st), scene=torch.zeros(n * steps, dtype=torch.int64))
    import pandas as pd
    df = tr.evaluate_rollout("f.csv", data, 0, steps, dt, pd.DataFrame(columns=trainer.ROLLOUT_COLUMNS))
    assert list(df.columns) == trainer.ROLLOUT_COLUMNS and len(df) == n * steps
    assert (df["step"].values == np.repeat(np.arange(steps), n)).all() and (df["step_time"] > 0).all()
    for c in ("x", "vx", "ax"):
        err = np.abs(df[c].astype(float) - df[f"pred_{c}"].astype(float)).max()
        assert err < 1e-4 * np.abs(df[c].astype(float)).max()
    mse = trainer.rollout_mse(df)
    assert len(mse) == steps and (mse["pos_mse"] < 1e-10).all()


def test_test_from_dir_on_a_generated_csv(tmp_path, gpu_device):
    """End to end: a dataset CSV in the reference's wire format (s01-dataset-generation.py:108-125)
    written from the HIP integrator -> datautils -> Trainer.test_from_dir -> the reference's two
    result frames (trainer.py:197-200)."""
    import csv
    import importlib.util
    import gnn
    import trainer
    from conftest import PKG
    steps, dt = 5, 0.01
    path = tmp_path / "data"
    path.mkdir()
    spec = importlib.util.spec_from_file_location("s01", f"{PKG}/s01-dataset-generation.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    out_csv = str(path / "output_file_1.csv")
    cli.main(["--integrator", "leapfrog", "--n-bodies", "20", "33", "--sim-type", "spiral", "--steps", str(steps),
              "--dt", str(dt), "--g", "1.0", "--softening", "0.1", "--seed", "3", "--output", out_csv, "--device", "cuda"])
    rows = list(csv.DictReader(open(out_csv, newline="")))
    assert list(rows[0].keys()) == cli.FIELDNAMES and len(rows) == (20 + 33) * steps
    assert {r["scene"] for r in rows} == {"0", "1"} and rows[0]["scene_type"] == "spiral" and rows[0]["step"] == "0"
    assert float(rows[0]["mass"]) == pytest.approx(0.01) and abs(float(rows[0]["x"])) < 1e-3   # body 0 = central black hole
    torch.manual_seed(0)
    model = gnn.GraphModel(input_dim=4, gnn_dim=16, message_passing_steps=2, aggr="mean", neighbors=4, device="cuda")
    tr = trainer.Trainer(model, optimizer=None, device="cuda", dt=dt)
    df_step, df_roll = tr.test_from_dir(str(path), sim_steps=steps)
    assert list(df_step.columns) == ["loss", "step_time"] and len(df_step) == 2
    assert list(df_roll.columns) == ["pos_rmse", "vel_rmse", "acc_rmse"] and len(df_roll) == 2 * steps
    assert np.isfinite(df_roll.values).all() and (df_roll.loc[("output_file_1.csv", 0, 0)][["pos_rmse", "vel_rmse"]] == 0).all()


@pytest.mark.parametrize("kind", ["gnn", "gnn64", "gnn64_separate_kick_drift", "gnn64_one_layer", "gnn64_one_layer_no_tables", "contconv"])
def test_hipgraph_rollout_step_equals_eager(kind, gpu_device):
    """Trainer._capture_step replays the captured step several times (state advances inside the graph);
    every replay must equal the eager Trainer.step bit for bit -- in particular counters that are
    zeroed inside the captured region have to be re-zeroed on every replay. gnn64: the published width, whose
    captured step has no kick-drift launch (the last layer's epilogue does the leapfrog bookkeeping, rounding as the
    separate kernels do); gnn64_separate_kick_drift: the same model with that form switched off. gnn64_one_layer(_no_tables):
    message_passing_steps = 1 -- the only layer launch gathers its neighbours' rows from the position array itself, which the
    pre-advancing epilogue would overwrite under the other workgroups' feet: the library refuses that form (NBD_E_UNSUPPORTED)
    and the captured step keeps its kick-drift launch; with the exponential tables off the edge loop really reads those rows."""
    import contconv
    import gnn
    import trainer
    torch.manual_seed(5)
    if kind.startswith("gnn"):
        model = gnn.GraphModel(input_dim=4, gnn_dim=32 if kind == "gnn" else 64,
                               message_passing_steps=1 if "one_layer" in kind else 2, aggr="mean", neighbors=10, device="cuda")
        if kind.endswith("no_tables"):
            model.use_exp_tables = False
    else:
        model = contconv.ContinuousConvModel(in_channels=4, out_channels=3, filter_resolution=[4, 3], radius=1.0, agg="mean",
                                             continuous_conv_layers=2, continuous_conv_dim=16, encoder_hiddens=[8],
                                             decoder_hiddens=[8], device="cuda").eval()
    tr = trainer.Trainer(model, None, device="cuda", dt=0.01)
    tr.pre_advance = kind != "gnn64_separate_kick_drift"
    pos, vel, m = _plummer_pos(900, 21)
    pos, vel, m1 = pos.cuda(), vel.cuda(), (m * 900)[:, None].cuda()
    acc = model.predict(pos, torch.cat([vel, m1], 1))
    adv = tr._capture_step(pos, vel, m1, acc, 0.01)
    assert adv is not None
    if kind.startswith("gnn"):
        assert model._advance_done == (kind == "gnn64")
        assert tr.last_capture == ("pre_advance" if kind == "gnn64" else "packed")
        assert model.last_path.startswith("one_call") and model.last_path.endswith("+pre_advance") == (kind == "gnn64")
        assert ("+tables" in model.last_path) == (not kind.endswith("no_tables"))
    else:
        assert model.last_path == ("fused", "fused") and tr.last_capture == "packed"
    p, v, a = pos, vel, acc
    for i in range(4):
        p, v, a = tr.step(p, v, m1, a, 0.01)
        gp, gv, ga = adv()
        assert torch.equal(gp, p) and torch.equal(gv, v) and torch.equal(ga, a), (kind, i)


@pytest.mark.parametrize("n", [1, 2, 5, 65])
def test_tiny_systems_match_oracle(n, gpu_device):
    """Degenerate sizes: a lone body has no kNN edges (EdgeConv -> 0, the head still sees LayerNorm of
    [x || 0]) and only its self-loop in the radius graph; k larger than n-1; fewer bodies than a wave."""
    import contconv
    import gnn
    from oracle import surrogate_oracle as so
    torch.manual_seed(n)
    pos, vel, m = _plummer_pos(max(n, 2), 30 + n)
    pos, vel, m = pos[:n].contiguous(), vel[:n].contiguous(), m[:n].contiguous()
    feat = torch.cat([vel, m[:, None]], 1)
    for width in (16, 64):                      # 64: the workgroup-of-16-nodes layer kernel with fewer nodes than that
        ora = so.GraphModelOracle(input_dim=4, gnn_dim=width, message_passing_steps=2, aggr="mean", neighbors=3).eval()
        model = gnn.GraphModel(input_dim=4, gnn_dim=width, message_passing_steps=2, aggr="mean", neighbors=3, device="cuda")
        _copy_state(model, ora)
        for fused in (True, False):
            model.use_fused = fused
            ref = ora.predict(pos, feat, k=50)
            for call in range(3 if fused else 1):   # later calls: the hinted one-call pass (staged search, tables)
                got = model.predict(pos.cuda(), feat.cuda()).cpu()
                assert got.shape == (n, 3) and torch.isfinite(got).all()
                assert (got - ref).abs().max() < 2e-5 * max(ref.abs().max().item(), 1.0), (width, fused, call)
    cfg = dict(in_channels=4, out_channels=3, filter_resolution=[3], radius=1.0, agg="mean", self_loops=True,
               continuous_conv_layers=1, continuous_conv_dim=8, encoder_hiddens=[6], decoder_hiddens=[5])
    ora_c = so.ContinuousConvModelOracle(**cfg).eval()
    mod_c = contconv.ContinuousConvModel(device="cuda", **cfg)
    _copy_state(mod_c, ora_c)
    got = mod_c.predict(pos.cuda(), feat.cuda()).cpu()
    ref = ora_c.predict(pos, feat)
    assert got.shape == (n, 3) and (got - ref).abs().max() < 2e-5 * max(ref.abs().max().item(), 1.0)
    # no self loops: an isolated body aggregates nothing (scatter mean of an empty set = 0)
    cfg["self_loops"] = False
    ora_n = so.ContinuousConvModelOracle(**cfg).eval()
    mod_n = contconv.ContinuousConvModel(device="cuda", **cfg)
    _copy_state(mod_n, ora_n)
    far = pos * 100.0
    assert (mod_n.predict(far.cuda(), feat.cuda()).cpu() - ora_n.predict(far, feat)).abs().max() < 2e-5


def test_trained_gnn_fixture_rollout(gpu_device):
    """The briefly-trained GNN (tests/golden/gnn_small_trained.pt, fitted on CPU by
    tests/golden/train_small_gnn.py with the oracle modules) loaded into the HIP model through the
    reference's state_dict layout: same predictions as the oracle with those weights, a step-wise error no
    worse than predicting zero on a held-out galaxy, and a finite, small rollout error."""
    import os
    import gnn
    import trainer
    import pandas as pd
    from conftest import GOLDEN_DIR
    from galaxify import galaxies
    from nbd.data import Data
    from oracle import galaxify_oracle as go
    from oracle import surrogate_oracle as so
    sd = torch.load(os.path.join(GOLDEN_DIR, "gnn_small_trained.pt"))
    ora = so.GraphModelOracle(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", neighbors=10).eval()
    ora.load_state_dict(sd)
    model = gnn.GraphModel(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", neighbors=10, device="cuda")
    model.load_state_dict(sd)
    n, steps, dt = 100, 20, 1e-4
    p, v, m = galaxies.generate_spiral(n_bodies=n, total_mass=1.0, radial_scale=3.0, height_scale=0.3, g_const=4.5e-6,
                                       black_hole_mass=0.01, seed=555)
    sim = go.OracleSimulator(positions=p, velocities=v, masses=m, g_const=4.5e-6, softening=0.05, dt=dt)
    m1 = sim.masses[:, None]
    xs, ys, st = [], [], []
    for s in range(steps):
        sim.leapfrog_step()
        xs.append(torch.cat([sim.positions, sim.velocities, m1], 1).clone()); ys.append(sim.accelerations.clone())
        st.append(torch.full((n,), s))
    x0, y0 = xs[0], ys[0]
    ref = ora.predict(x0[:, :3].contiguous(), x0[:, 3:].contiguous(), k=50)
    got = model.predict(x0[:, :3].contiguous().cuda(), x0[:, 3:].contiguous().cuda()).cpu()
    assert global_rel(got, ref) < 1e-4                       # tiny outputs (1e-7): looser than the 1e-5 of O(1) tests
    err = (got - y0).pow(2).mean().sqrt().item()
    assert err < 1.5 * y0.pow(2).mean().sqrt().item()        # the fit is at the reference's own level (RMSE ~ signal)
    data = Data(x=torch.cat(xs), y=torch.cat(ys), step=torch.cat(st))
    tr = trainer.Trainer(model, None, device="cuda", dt=dt)
    df = tr.evaluate_rollout("f.csv", data, 0, steps, dt, pd.DataFrame(columns=trainer.ROLLOUT_COLUMNS))
    mse = trainer.rollout_mse(df)
    assert np.isfinite(mse.values).all() and mse["pos_mse"].iloc[-1] < 1e-12 and mse["vel_mse"].iloc[-1] < 1e-8


# ------------------------------------------------------------------ pinned by vectors from the reference's own classes
def _ref_vectors(name):
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", f"surrogate_ref_{name}.npz"), allow_pickle=False)


@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_contconv_public_helpers_reproduce_the_reference_class(case, gpu_device):
    """ContinuousConv.ball_to_cube / .trilinear_interpolate (contconv.py:30-33, 53-78) on the drop-in layer against the
    outputs of the reference's own methods (tests/golden/surrogate_ref_contconv.npz, make_golden_surrogate.py): the mapped
    offsets, the (N, I, O) blends at stored grid coordinates, and the composition the layer's forward uses."""
    import contconv
    g = _ref_vectors("contconv")
    filters = torch.tensor(g[f"c{case}_filters"])
    d, i, o = filters.shape[0], filters.shape[3], filters.shape[4]
    layer = contconv.ContinuousConv(i, o, d, radius=1.0).cuda()
    with torch.no_grad():
        layer.filters.copy_(filters.cuda())
    r = torch.tensor(g[f"c{case}_r"]).cuda()
    cube = layer.ball_to_cube(r)
    assert cube.shape == r.shape and float((cube.cpu() - torch.tensor(g[f"c{case}_cube"])).abs().max()) <= 2e-7
    coords = torch.tensor(g[f"c{case}_coords"]).cuda()
    got = layer.trilinear_interpolate(coords)
    ref = torch.tensor(g[f"c{case}_interp"])
    assert got.shape == ref.shape and float((got.cpu() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
    grid = (cube + 1) * ((d - 1) / 2)                                              # contconv.py:89-90
    got_r = layer.trilinear_interpolate(grid)
    ref_r = torch.tensor(g[f"c{case}_interp_of_r"])
    assert float((got_r.cpu() - ref_r).abs().max()) <= 1e-5 * max(1.0, float(ref_r.abs().max()))
    assert layer.trilinear_interpolate(coords[:0]).shape == (0, i, o) and layer.ball_to_cube(r[:0]).shape == (0, 3)


@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_contconv_kernels_reproduce_reference_interpolation(case, gpu_device):
    """48 isolated edges (target t_k, source s_k = t_k + r_k): the HIP binning + GEMM must give
    window_k * sum_i filt_k[i][:] feat[s_k][i] with filt_k = the REFERENCE's trilinear_interpolate(
    (ball_to_cube(r_k) + 1)(D-1)/2) as stored by tests/golden/make_golden_surrogate.py (contconv.py:84-93).
    (The stronger pin -- the reference's whole forward on dense graphs, every path, at the reference's own fp32 error:
    test_contconv_forward_reproduces_the_reference_run below.)"""
    import contconv
    g = _ref_vectors("contconv")
    filters = torch.tensor(g[f"c{case}_filters"])
    r = torch.tensor(g[f"c{case}_r"])
    filt = torch.tensor(g[f"c{case}_interp_of_r"]).double()                # (48, I, O)
    d, i, o = filters.shape[0], filters.shape[3], filters.shape[4]
    k = r.shape[0]
    gen = torch.Generator().manual_seed(case)
    base = torch.randn(k, 3, generator=gen) * 5
    pos = torch.cat([base, base + r])                                      # targets 0..k-1, sources k..2k-1
    r_eff = (pos[k:] - pos[:k])                                            # what the kernel sees (fp32 rounding of base + r)
    feat = torch.randn(2 * k, i, generator=gen)
    ei = torch.stack([torch.arange(k), torch.arange(k) + k])               # row = target, col = source
    layer = contconv.ContinuousConv(i, o, d, radius=1.0, agg="sum").cuda()
    with torch.no_grad():
        layer.filters.copy_(filters.cuda())
        got = layer(pos.cuda(), feat.cuda(), edge_index=ei.cuda()).cpu().double()
    d2 = (r_eff.double() ** 2).sum(-1)
    window = ((1 - d2) ** 3) * (d2 < 1.0)
    ref = torch.einsum("eio,ei->eo", filt, feat[k:].double()) * window[:, None]
    # base + r is rounded to fp32, so r_eff differs from the stored r by ~1e-7 * |base|: compare only the edges
    # where that perturbation is negligible against |r| (the others are covered by the oracle tests)
    ok = (r_eff - r).norm(dim=1) <= 1e-4 * r.norm(dim=1).clamp(min=1e-30)
    assert ok.sum() >= k // 2
    err = (got[:k][ok] - ref[ok]).norm() / ref[ok].norm()
    assert err < 2e-4, err                                                  # interpolation argument perturbed by <= 1e-4 rel
    assert float(got[k:].abs().max()) == 0.0                               # sources receive nothing


# ContinuousConv.forward pinned by the reference's own fp64 run up to its scatter call (tests/contconv_pin_cases.py,
# tests/golden/surrogate_ref_contconv_forward_*.npz; the host side of the pin: tests/test_surrogate_oracle.py)
def _pin_case(case, agg=None):
    """(layer, pos, feat, edge_index on the GPU, rows that must be exactly 0.0, inputs) of a pinned case."""
    import contconv
    import contconv_pin_cases as pc
    n, d, i, o, case_agg, radius, _, _ = pc.CASES[case]
    inp = pc.checked_inputs(case)
    layer = contconv.ContinuousConv(i, o, d, radius=radius, agg=agg or case_agg).cuda()
    with torch.no_grad():
        layer.filters.copy_(torch.from_numpy(inp["filters"]).cuda())
    ei = inp["edge_index"]
    rel = inp["pos"].astype(np.float64)[ei[1]] - inp["pos"].astype(np.float64)[ei[0]]
    inside = ((rel ** 2).sum(1) < radius ** 2).astype(np.float64)               # exact: the lattice (contconv_pin_cases)
    zero_rows = torch.from_numpy(np.bincount(ei[0], weights=inside, minlength=n) == 0)   # no edge, or none inside the radius
    return layer, torch.from_numpy(inp["pos"]).cuda(), torch.from_numpy(inp["feat"]).cuda(), torch.from_numpy(ei).cuda(), zero_rows, inp


def _exactly_zero(got, zero_rows):
    return not zero_rows.any() or float(got.cpu()[zero_rows].abs().max()) == 0.0


@pytest.mark.parametrize("case", ["f0", "f1", "f2", "f3", "f4", "f5"])
def test_contconv_forward_reproduces_the_reference_run(case, gpu_device):
    """Inference through edge_index= on the fused and the binned path against out64, the reference's own fp64 run of
    forward (contconv.py:80-98) on a dense, permuted edge list with duplicates, edges beyond the radius, a coincident pair
    and a pair at exactly the radius. Bars: the project's, and four times the reference's own fp32 error."""
    import contconv_pin_cases as pc
    layer, pos, feat, ei, zero_rows, _ = _pin_case(case)
    assert layer.fused_ok()
    with torch.no_grad():
        got = layer(pos, feat, edge_index=ei)
        assert layer.last_path == "fused"
        again = layer(pos, feat, edge_index=ei)
        by_target = layer(pos, feat, edge_index=ei[:, torch.sort(ei[0], stable=True).indices])
        layer.use_fused = False
        old = layer(pos, feat, edge_index=ei)
        assert layer.last_path == "binned"
        old_again = layer(pos, feat, edge_index=ei)
    pc.check(got.cpu().numpy(), case, "out", "fused")
    pc.check(old.cpu().numpy(), case, "out", "binned")
    assert torch.equal(got, again) and torch.equal(old, old_again)             # a second call gives the same bits
    assert torch.equal(got, by_target)                                         # the layer sorts stably by target
    assert _exactly_zero(got, zero_rows) and _exactly_zero(old, zero_rows)


def test_contconv_extreme_aggregation_reproduces_the_reference_run(gpu_device):
    """f6 (max, no self loops): rows without edges and rows whose every listed edge is beyond the radius are exactly 0.0 --
    also under sum and mean on the fused and the binned path, where an edge beyond the radius still counts in the mean."""
    import contconv_pin_cases as pc
    layer, pos, feat, ei, zero_rows, inp = _pin_case("f6")
    deg = np.bincount(inp["edge_index"][0], minlength=pos.shape[0])
    assert (deg == 0).any() and (zero_rows.numpy() & (deg > 0)).any()
    with torch.no_grad():
        got = layer(pos, feat, edge_index=ei)
        assert layer.last_path == "extreme"
        again = layer(pos, feat, edge_index=ei)
    pc.check(got.cpu().numpy(), "f6", "out", "extreme")
    assert torch.equal(got, again) and _exactly_zero(got, zero_rows)
    for agg in ("sum", "mean"):
        lin, _, _, _, _, _ = _pin_case("f6", agg=agg)
        for fused in (True, False):
            lin.use_fused = fused
            with torch.no_grad():
                out = lin(pos, feat, edge_index=ei)
            assert lin.last_path == ("fused" if fused else "binned") and _exactly_zero(out, zero_rows)
            assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0.0


@pytest.mark.parametrize("case", ["f1", "f2", "f5"])
def test_contconv_forward_through_the_search_lists_reproduces_the_reference_run(case, gpu_device):
    """Inference through lists= (graphops.radius_lists on the same positions): the search's edges agree index for index with
    the radius-graph part of the stored edge list, and the output with out64_lists, the reference's messages of those edges."""
    import contconv_pin_cases as pc
    from nbd import graphops
    layer, pos, feat, ei, _, _ = _pin_case(case)
    _, _, _, _, _, radius, cap, loop = pc.CASES[case]
    stored = ei[:, torch.from_numpy(pc.fixture()[f"{case}_radius_at"].astype(np.int64)).cuda()]
    assert torch.equal(graphops.radius_graph(pos, radius, None, loop=loop, max_num_neighbors=cap), stored)
    lists = graphops.radius_lists(pos, radius, None, loop=loop, max_num_neighbors=cap)
    e = stored.shape[1]
    order = torch.sort(stored[0], stable=True).indices                          # CSR by aggregation target, centres ascending
    assert int(lists.rowptr[-1]) == e and torch.equal(lists.centres[:e].long(), stored[1][order])
    assert torch.equal(lists.rowptr.long(), torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"),
                                                        torch.cumsum(torch.bincount(stored[0], minlength=pos.shape[0]), 0)]))
    with torch.no_grad():
        got = layer(pos, feat, lists=lists)
        assert layer.last_path == "fused"
        layer.use_fused = False
        old = layer(pos, feat, lists=lists)
        assert layer.last_path == "binned"
    pc.check(got.cpu().numpy(), case, "out_lists", "fused, lists=")
    pc.check(old.cpu().numpy(), case, "out_lists", "binned, lists=")


def test_contconv_tanh_epilogue_and_strided_output_reproduce_the_reference_run(gpu_device):
    """f2 with act="tanh" (the model's next operation, contconv.py:228-230) and with out= a column view of a wider buffer."""
    import contconv_pin_cases as pc
    layer, pos, feat, ei, _, _ = _pin_case("f2")
    n, i, o = pos.shape[0], layer.in_channels, layer.out_channels
    for fused in (True, False):
        layer.use_fused = fused
        path = "fused" if fused else "binned"
        buf = torch.zeros((n, i + o + 2), device="cuda")          # how the model passes its concatenation buffer
        with torch.no_grad():
            got = layer(pos, feat, edge_index=ei)
            got_t = layer(pos, feat, edge_index=ei, act="tanh")
            assert layer.last_path == path
            layer(pos, feat, edge_index=ei, out=buf[:, i:i + o])
            assert layer.last_path == path
        pc.check(got_t.cpu().numpy(), "f2", "tanh", path)
        assert torch.equal(buf[:, i:i + o], got)
        assert float(buf[:, i + o:].abs().max()) == 0.0 and float(buf[:, :i].abs().max()) == 0.0


def test_trainer_rollout_reproduces_reference_frame(gpu_device):
    """Trainer.step / evaluate_rollout against the frame the REFERENCE's Trainer class produced for the same
    data and an fp32-exact toy model (tests/golden/make_golden_surrogate.py): identical columns, bit-identical
    predicted positions / velocities / accelerations and ground-truth columns."""
    import pandas as pd
    import trainer
    from nbd.data import Data
    g = _ref_vectors("trainer")

    class Toy(torch.nn.Module):
        neighbors = 0

        def predict(self, pos, feat):
            return (feat[:, 3:4] * (-pos)) * 0.5 + feat[:, :3] * 0.25
    tr = trainer.Trainer(Toy(), None, device="cuda", dt=float(g["dt"]))
    pos, vel, m, acc = (torch.tensor(g[k]).cuda() for k in ("pos", "vel", "m", "acc"))
    p1, v1, a1 = tr.step(pos, vel, m, acc, float(g["dt"]))
    assert np.array_equal(p1.cpu().numpy(), g["step_pos"]) and np.array_equal(v1.cpu().numpy(), g["step_vel"])
    assert np.array_equal(a1.cpu().numpy(), g["step_acc"])
    data = Data(x=torch.tensor(g["data_x"]).cuda(), y=torch.tensor(g["data_y"]).cuda(), step=torch.tensor(g["data_step"]).cuda())
    steps = int(g["data_step"].max()) + 1
    for use_graph in (True, False):
        tr.use_hip_graph = use_graph
        df = tr.evaluate_rollout("file.csv", data, 3, steps, float(g["dt"]), pd.DataFrame())
        assert list(df.columns) == list(g["rollout_columns"])
        cols = list(g["rollout_numeric_columns"])
        assert np.array_equal(df[cols].to_numpy(dtype=np.float64), g["rollout_values"]), use_graph
        assert df["filename"].tolist() == list(g["rollout_filename"])


def _write_toy_csv(path, rows):
    """The dataset CSV layout of s01-dataset-generation.py:108-125 from (R, 12) rows holding fp32 values."""
    with open(path, "w") as f:
        f.write("scene,scene_type,step,step_time,mass,x,y,z,vx,vy,vz,ax,ay,az,u,k\n")
        for r in rows:
            f.write(",".join([str(int(r[0])), "toy", str(int(r[1])), "0.0"] + [repr(float(v)) for v in r[2:]]
                             + ["0.0", "0.0"]) + "\n")


@pytest.mark.parametrize("use_graph,together", [(False, False), (True, False), (False, True), (True, True)])
def test_test_from_dir_reproduces_reference_frames(use_graph, together, tmp_path, gpu_device):
    """Trainer.test_from_dir / evaluate_stepwise against the two frames the REFERENCE's Trainer class
    returned for the same CSV files and an fp32-exact toy model (tests/golden/make_golden_surrogate.py):
    pos/vel/acc_rmse = sqrt(mean_xyz(mean signed error^2)) per (file, scene, step) and the mean loss per
    (file, scene) (trainer.py:177-200). Here the CSVs go through the product's datautils (kNN on the GPU) and
    the rollout through the HIP kick/drift kernels, eager and as a captured hipGraph; `together`: the toy model also offers
    predict_batched, so all scenes of a file advance as ONE batched system (Trainer.evaluate_rollout_scenes) -- same frames."""
    import trainer
    g = _ref_vectors("test_from_dir")
    for key in g.files:
        if key.startswith("csv_") and key != "csv_columns":
            _write_toy_csv(tmp_path / f"{key[4:]}.csv", g[key])

    class Toy(torch.nn.Module):
        neighbors = 3

        def predict(self, pos, feat):
            return (feat[:, 3:4] * (-pos)) * 0.5 + feat[:, :3] * 0.25

        def eval_graph_batch(self, data):
            pred = self.predict(data.x[:, :3], data.x[:, 3:])
            mse = ((pred - data.y) ** 2).mean()
            return mse.sqrt().item(), mse.item(), 0.125
    if together:
        Toy.predict_batched = lambda self, pos, feat, batch: self.predict(pos, feat)       # per-body arithmetic: no graph to split
    tr = trainer.Trainer(Toy(), None, device="cuda", dt=float(g["dt"]))
    tr.use_hip_graph = use_graph
    steps = int(g["sim_steps"])
    tr.hip_graph_min_steps = 2         # the fixture has 4 steps: capture anyway
    df_step, df_roll = tr.test_from_dir(str(tmp_path), sim_steps=steps)
    modes = {m for _, m in tr.last_rollout_modes}
    assert modes == ({"2 scenes together", "scene by scene"} if together else {"scene by scene"})      # a 2-scene and a 1-scene file
    df_step, df_roll = df_step.sort_index(), df_roll.sort_index()
    assert list(df_step.columns) == list(g["stepwise_columns"]) and list(df_roll.columns) == list(g["rollout_columns"])
    assert [i[0] for i in df_step.index] == list(g["stepwise_index_filename"])
    assert [int(i[1]) for i in df_step.index] == list(g["stepwise_index_scene"])
    assert [i[0] for i in df_roll.index] == list(g["rollout_index_filename"])
    assert [int(i[1]) for i in df_roll.index] == list(g["rollout_index_scene"])
    assert [int(i[2]) for i in df_roll.index] == list(g["rollout_index_step"])
    # stepwise: `loss` is the toy model's own fp32 .mean() over a graph (reduction order differs CPU vs GPU:
    # ~1e-7), averaged per scene by the trainer; step_time is the constant the model returns
    assert np.allclose(df_step.to_numpy(dtype=np.float64), g["stepwise_values"], rtol=1e-6, atol=0)
    # rollout: per-row values are fp32-exact on both sides; the float64 group means may associate differently
    assert np.allclose(df_roll.to_numpy(dtype=np.float64), g["rollout_values"], rtol=1e-9, atol=1e-15)
    assert (g["rollout_values"][:, 2] > 0).all() and g["rollout_values"][0, 0] == 0      # a real, non-trivial frame


@pytest.mark.parametrize("kind", ["gnn", "contconv"])
def test_scenes_advanced_together_match_scenes_advanced_one_by_one(kind, gpu_device):
    """Trainer.evaluate_rollout_scenes / model.predict_batched: three scenes of 3, 40 and 200 bodies as ONE batched system
    (neighbour searches inside a scene only) against the same scenes rolled out one after another -- the first prediction
    to 1e-5 (same kernels, CSR form), the frames' shape and bookkeeping exactly, eager and captured."""
    import contconv
    import gnn
    import trainer
    from nbd.data import Data
    torch.manual_seed(9)
    if kind == "gnn":
        model = gnn.GraphModel(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", neighbors=10, device="cuda")
        model.use_one_call = False                   # scene by scene through the per-kernel layers too: the same arithmetic
    else:
        model = contconv.ContinuousConvModel(in_channels=4, out_channels=3, filter_resolution=[4, 3], radius=1.0, agg="mean",
                                             continuous_conv_layers=2, continuous_conv_dim=16, encoder_hiddens=[8],
                                             decoder_hiddens=[8], device="cuda").eval()
        model.use_radius_cache = False
    sizes, steps, dt = [3, 40, 200], 4, 0.01
    scenes = []
    for i, n in enumerate(sizes):
        p, v, m = _plummer_pos(max(n, 4), 50 + i)
        x0 = torch.cat([p[:n], v[:n], (m[:n] * n)[:, None]], 1)
        x = torch.cat([x0 + 0.01 * s for s in range(steps)])            # ground truth rows: arbitrary but step-tagged
        scenes.append(Data(x=x.cuda(), y=torch.randn(steps * n, 3).cuda(), step=torch.arange(steps).repeat_interleave(n).cuda(),
                           scene=torch.full((steps * n,), i).cuda()))
    pos = torch.cat([d.x[:n, :3] for d, n in zip(scenes, sizes)]).contiguous()
    feat = torch.cat([d.x[:n, 3:] for d, n in zip(scenes, sizes)]).contiguous()
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(sizes)).cuda()
    together = model.predict_batched(pos, feat, batch)
    one_by_one = torch.cat([model.predict(d.x[:n, :3].contiguous(), d.x[:n, 3:].contiguous()) for d, n in zip(scenes, sizes)])
    assert global_rel(together.cpu(), one_by_one.cpu()) < TOL and row_rel(together.cpu(), one_by_one.cpu()) < 10 * TOL
    for use_graph in (False, True):
        tr = trainer.Trainer(model, None, device="cuda", dt=dt)
        tr.use_hip_graph, tr.hip_graph_min_steps = use_graph, 2
        df_t = tr.evaluate_rollout_scenes("f.csv", scenes, steps, dt, None)
        assert tr.last_rollout_timing["scenes_together"] == 3 and tr.last_rollout_timing["captured"] == use_graph
        df_s = None
        for i, d in enumerate(scenes):
            df_s = tr.evaluate_rollout("f.csv", d, i, steps, dt, df_s)
        assert list(df_t.columns) == list(df_s.columns) and len(df_t) == len(df_s) == steps * sum(sizes)
        for c in ("filename", "scene", "step", "x", "vz", "az"):
            assert (df_t[c].to_numpy() == df_s[c].to_numpy()).all(), c
        a, b = df_t[["pred_x", "pred_y", "pred_z"]].to_numpy(), df_s[["pred_x", "pred_y", "pred_z"]].to_numpy()
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max()


def test_evaluate_rollout_rejects_ragged_steps(gpu_device):
    """A batch whose steps do not all hold the bodies of step 0 cannot be rolled out (the reference indexes the
    ground truth by prediction row and fails with an IndexError there); here it is reported up front."""
    import pandas as pd
    import trainer
    from nbd.data import Data

    class Toy(torch.nn.Module):
        def predict(self, pos, feat):
            return -pos
    tr = trainer.Trainer(Toy(), None, device="cuda", dt=0.01)
    x = torch.randn(11, 7).cuda()
    data = Data(x=x, y=torch.randn(11, 3).cuda(), step=torch.tensor([0] * 4 + [1] * 4 + [2] * 3).cuda())
    with pytest.raises(ValueError):
        tr.evaluate_rollout("f.csv", data, 0, 3, 0.01, pd.DataFrame())


@pytest.mark.parametrize("n,k", [(500, 10), (4096, 50), (700, 70), (65, 64), (6000, 30)])
def test_knn_graph_result_does_not_depend_on_the_hint(n, k, gpu_device):
    """nbd_knn_graph_hint_f32: a previous graph bounds the search; a perfect, stale, duplicated or garbage hint
    must all give exactly the un-hinted (= oracle) result, also when the hint buffer is the output buffer."""
    from nbd import graphops
    from oracle import surrogate_oracle as so
    pos, vel, _ = _plummer_pos(n, 30 + n)
    ref = so.knn_graph(pos, k)
    kk = min(k, n - 1)
    g = torch.Generator().manual_seed(n)
    moved = pos + 0.05 * vel                                            # "the next rollout step"
    ref_moved = so.knn_graph(moved, k)
    good = ref.clone()
    dup = ref.clone(); dup[0] = dup[0].reshape(n, kk)[:, :1].expand(n, kk).reshape(-1)      # one neighbour repeated kk times
    garbage = torch.stack([torch.randint(-5, n + 5, (n * kk,), generator=g), ref[1]])
    selfs = torch.stack([ref[1].clone(), ref[1]])                       # every hint is the centre itself
    far = torch.stack([torch.randint(0, n, (n * kk,), generator=g), ref[1]])   # random (mostly distant) nodes
    for name, hint in (("good", good), ("dup", dup), ("garbage", garbage), ("self", selfs), ("far", far)):
        got = graphops.knn_graph(moved.cuda(), k, hint=hint.cuda().contiguous())
        assert torch.equal(got.cpu(), ref_moved), name
    buf = graphops.knn_graph(pos.cuda(), k)
    assert torch.equal(buf.cpu(), ref)
    out = graphops.knn_graph(moved.cuda(), k, hint=buf, out=buf)        # in place: hint and output share the buffer
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf.cpu(), ref_moved)


def test_gnn_predict_reuses_its_previous_graph_as_hint(gpu_device):
    import gnn
    from oracle import surrogate_oracle as so
    torch.manual_seed(2)
    ora = so.GraphModelOracle(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", neighbors=10).eval()
    model = gnn.GraphModel(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", neighbors=10, device="cuda")
    _copy_state(model, ora)
    pos, vel, m = _plummer_pos(600, 6)
    feat = torch.cat([vel, m[:, None] * 600], 1)
    for step in range(3):                                               # second and third call run hinted, in place
        p = pos + 0.02 * step * vel
        assert global_rel(model.predict(p.cuda(), feat.cuda()).cpu(), ora.predict(p, feat, k=50)) < TOL, step
    other, _, _ = _plummer_pos(600, 99)                                 # an unrelated system of the same size
    assert global_rel(model.predict(other.cuda(), feat.cuda()).cpu(), ora.predict(other, feat, k=50)) < TOL


# ------------------------------------------------------------------ BASELINE configs[2] / [3] at their full sizes
def test_gnn_full_size_config_matches_oracle(gpu_device):
    """configs[2]: published GNN shape, N = 4096, k = 32 -- the whole forward against the oracle at full size."""
    import gnn
    from oracle import surrogate_oracle as so
    torch.manual_seed(7)
    cfg = dict(input_dim=4, gnn_dim=64, message_passing_steps=2, aggr="mean", neighbors=10)
    ora = so.GraphModelOracle(**cfg).eval()
    model = gnn.GraphModel(device="cuda", **cfg)
    _copy_state(model, ora)
    n = 4096
    pos, vel, m = _plummer_pos(n, 1234)
    feat = torch.cat([vel, m[:, None] * n], 1)
    ref = ora.predict(pos, feat, k=32)
    got = model.predict(pos.cuda(), feat.cuda(), neighbors=32).cpu()
    assert global_rel(got, ref) < TOL and row_rel(got, ref) < 10 * TOL
    # the first call already takes the one-call pass (hinted search in place, tanh through the exponential tables), so
    # predict() is idempotent: the same input gives the same bits call after call
    assert model._one_call is not None and model._one_call["fa"].workspace_bytes > 0
    assert model.last_path == "one_call+tables"                                   # the fast path was taken, and says so
    for _ in range(2):
        assert torch.equal(model.predict(pos.cuda(), feat.cuda(), neighbors=32).cpu(), got)
    model.use_exp_tables, model._one_call = False, None                           # without the tables: exact tanh
    plain = model.predict(pos.cuda(), feat.cuda(), neighbors=32).cpu()
    assert model.last_path == "one_call" and global_rel(plain, ref) < TOL and row_rel(plain, ref) < 10 * TOL
    model.use_one_call = False                                                    # one launch per layer: the same bits
    assert torch.equal(model.predict(pos.cuda(), feat.cuda(), neighbors=32).cpu(), plain) and model.last_path == "fused"
    model.use_fused = False                                                       # a forced fallback shows up, it is not silent
    slow = model.predict(pos.cuda(), feat.cuda(), neighbors=32).cpu()
    assert model.last_path == "general" and global_rel(slow, ref) < TOL


def test_contconv_full_size_config_rows_match_oracle_and_layer_is_linear(gpu_device):
    """configs[3]: published ContinuousConv layer shape (D = 6, 128 -> 128 channels) at N = 16 384 with a mean
    radius-1 degree of ~32. The oracle is too slow for all rows, so (a) 48 random rows are checked against the
    oracle evaluated on exactly the edges that end in them, (b) the layer (no activation) must be linear in the
    features at full size: conv(a f1 + b f2) = a conv(f1) + b conv(f2)."""
    import contconv
    from nbd import graphops
    from oracle import surrogate_oracle as so
    torch.manual_seed(11)
    n, D, C = 16384, 6, 128
    pos, _, _ = _plummer_pos(n, 1234)
    pos = pos * 4.6                                                  # mean number of bodies within radius 1 ~ 32
    ora = so.ContinuousConvOracle(C, C, D, radius=1.0, agg="mean")
    layer = contconv.ContinuousConv(C, C, D, radius=1.0, agg="mean").cuda()
    _copy_state(layer, ora)
    f1, f2 = torch.randn(n, C), torch.randn(n, C)
    ei = graphops.radius_graph(pos.cuda(), 1.0, loop=True, max_num_neighbors=32)
    with torch.no_grad():
        o1 = layer(pos.cuda(), f1.cuda(), edge_index=ei)
        o2 = layer(pos.cuda(), f2.cuda(), edge_index=ei)
        o12 = layer(pos.cuda(), (0.5 * f1 - 2.0 * f2).cuda(), edge_index=ei)
        assert global_rel(o12.cpu(), (0.5 * o1 - 2.0 * o2).cpu()) < TOL
        rows = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:48]
        ei_c = ei.cpu()
        keep = torch.isin(ei_c[0], rows)                                 # aggregation happens at edge_index[0]
        ref = ora(pos, f1, ei_c[:, keep])[rows]
        assert float(ref.abs().max()) > 0
        assert global_rel(o1.cpu()[rows], ref) < TOL
    assert 10 < ei.shape[1] / n <= 32                                  # capped at 32 per centre (uncapped mean ~32)


@pytest.mark.parametrize("D", [6, 4])
@pytest.mark.parametrize("spread", ["normal", "2^-20..2^20"])
def test_contconv_bf16x3_contraction_error_is_no_larger_than_the_fp32_matrix_pipes(D, spread, gpu_device):
    """The fused kernel multiplies on the bf16 matrix pipe with both operands split into three bf16 terms (csrc/contconv_fused.hip).
    `dtype` stays "fp32" only if that is fp32-equivalent: on the published layer shape (N = 16 384, 128 -> 128 channels, D = 6
    and D = 4) the row error against an exact (fp64) product must be no larger than that of the fp32 matrix instruction
    on the same inputs -- the library's other ContinuousConv path (binned features + nbd_linear_f32, v_mfma_f32_16x16x4_f32).
    The graph isolates the contraction: bodies farther apart than the radius, self loops only, so every node reaches the
    eight cells around the grid centre with weight 1/8 (exact) and the exact result is feat . (sum of those filters) / 8.
    Inputs: N(0, 1), and magnitudes 2^u, u uniform in [-20, 20], random signs."""
    import contconv
    n, C = 16384, 128
    g = torch.Generator().manual_seed(1000 * D + len(spread))
    side = 26
    idx = torch.arange(n)
    pos = torch.stack((idx % side, (idx // side) % side, idx // (side * side)), 1).to(torch.float32) * 3.0     # spacing 3 > radius 1
    def draw(*shape):
        if spread == "normal":
            return torch.randn(*shape, generator=g)
        mag = torch.exp2(torch.rand(*shape, generator=g) * 40.0 - 20.0)
        return mag * (torch.randint(0, 2, shape, generator=g).to(torch.float32) * 2.0 - 1.0)
    feat = draw(n, C)
    layer = contconv.ContinuousConv(C, C, D, radius=1.0, agg="sum").cuda()
    with torch.no_grad():
        layer.filters.copy_(draw(D, D, D, C, C))
    ei = torch.stack((idx, idx)).cuda()                                       # self loops
    with torch.no_grad():
        assert layer.fused_ok()
        got = layer(pos.cuda(), feat.cuda(), edge_index=ei).cpu().double()
        layer.use_fused = False
        f32 = layer(pos.cuda(), feat.cuda(), edge_index=ei).cpu().double()
    c0 = D // 2 - 1                                                            # D even: |r| = 0 sits between cells c0 and c0 + 1 on every axis
    fsum = layer.filters.detach().cpu().double()[c0:c0 + 2, c0:c0 + 2, c0:c0 + 2].sum((0, 1, 2))
    ref = feat.double() @ fsum / 8.0
    scale = ref.abs().amax(1).clamp_min(1e-300)
    err_bf = ((got - ref).abs().amax(1) / scale)
    err_32 = ((f32 - ref).abs().amax(1) / scale)
    assert float(err_32.max()) < 1e-5 and float(err_bf.max()) < 1e-5           # both are fp32 products at all
    # no larger: in the worst row and on (quadratic) average over the 16 384 rows
    assert float(err_bf.max()) <= float(err_32.max()), (float(err_bf.max()), float(err_32.max()))
    assert float(err_bf.square().mean().sqrt()) <= float(err_32.square().mean().sqrt())


def test_contconv_stream_kernel_ranges_longer_than_one_table_pass(gpu_device):
    """A workgroup of the stream kernel copies <= 256 step records into LDS at a time; at the published size every range is
    shorter than that. N = 40 000 at D = 6 gives every workgroup ~500 steps of its cell group (three passes: the ring's
    counters run on across passes, the filter fragment is requested afresh at every pass start and drained at its end) and
    N = 40 000 at D = 3 (27 cells: ONE cell group, 256 workgroups) ranges that cross many tiles. Checked against the
    library's other path (binned features + fp32 GEMM) on every row, twice (deterministic)."""
    import contconv
    from nbd import graphops, nnops
    n = 40000
    pos, _, _ = _plummer_pos(n, 99)
    pos = (pos * 6.2).cuda()                                            # mean radius-1 degree ~ 32 at this size
    torch.manual_seed(4)
    feat = torch.randn(n, 32).cuda()
    lists = graphops.radius_lists(pos, 1.0, loop=True, max_num_neighbors=32)
    for D in (6, 3):
        layer = contconv.ContinuousConv(32, 32, D, radius=1.0, agg="mean").cuda()
        _, cmap, n_cells = layer.cells()
        pairs = nnops.contconv_pairs(pos, lists.rowptr, lists.centres, lists.centres.numel(), D, 1.0, cmap, n_cells)
        steps = nnops.contconv_pairs_stats(pairs[0], n, pairs[1], n_cells)["steps"]
        groups = 8 if n_cells >= 96 else 2 if n_cells >= 32 else 1
        if D == 6:
            assert steps / 256 > 2 * 256                                # every workgroup: more than two table passes
        with torch.no_grad():
            got = layer(pos, feat, lists=lists, act="tanh", pairs=pairs)
            assert layer.last_path == "fused"
            again = layer(pos, feat, lists=lists, act="tanh", pairs=pairs)
            layer.use_fused = False
            ref = layer(pos, feat, lists=lists, act="tanh")
        assert torch.equal(got, again)
        assert global_rel(got.cpu(), ref.cpu()) < TOL and row_rel(got.cpu(), ref.cpu()) < 10 * TOL, (D, groups)


BENCH_SCALE_16384 = 4.599349753792708      # tools/bench_surrogates.py: Plummer positions x this -> mean radius-1 degree 32


def test_radius_graph_index_exact_at_config_size(gpu_device):
    """configs[3]'s own size: radius_graph at N = 16 384 with the bench's position scale, every edge index
    against the oracle's brute force (2.7e8 distance tests on the host, row-blocked)."""
    from nbd import graphops
    from oracle import surrogate_oracle as so
    n = 16384
    pos, _, _ = _plummer_pos(n, 1234)
    pos = pos * BENCH_SCALE_16384
    ref = so.radius_graph(pos, 1.0, loop=True, max_num_neighbors=32)
    got = graphops.radius_graph(pos.cuda(), 1.0, loop=True, max_num_neighbors=32).cpu()
    assert got.shape == ref.shape and torch.equal(got, ref)
    assert ref.shape[1] == 277746                                  # the edge count the bench reports
    ref_nl = so.radius_graph(pos, 1.0, loop=False, max_num_neighbors=32)
    assert torch.equal(graphops.radius_graph(pos.cuda(), 1.0, loop=False, max_num_neighbors=32).cpu(), ref_nl)


def test_contconv_published_model_at_config_size_matches_oracle_rows(gpu_device):
    """configs[3] end to end: the PUBLISHED ContinuousConvModel (contconv_experiment.py:62-76: encoder MLP
    [4,32,64,128] with BatchNorm, two ContinuousConv layers 128 -> 128 with D = 6 and 4, LayerNorm, decoder
    [64,32] -> 3) at N = 16 384. The HIP model runs the whole system from its own radius search; the oracle
    evaluates a sample of rows exactly, on the ORACLE's edge list: layer 2 at the sampled rows needs layer 1 at
    their neighbours, which needs the encoder output at the neighbours' neighbours (the encoder is per node)."""
    import contconv
    from oracle import surrogate_oracle as so
    torch.manual_seed(21)
    n = 16384
    cfg = dict(in_channels=4, out_channels=3, filter_resolution=[6, 4], radius=1.0, agg="mean", self_loops=True,
               continuous_conv_layers=2, continuous_conv_dim=128, encoder_hiddens=[32, 64], decoder_hiddens=[64, 32])
    ora = so.ContinuousConvModelOracle(**cfg)
    with torch.no_grad():
        for nrm in ora.node_encoder.norms:
            nrm.module.running_mean.uniform_(-0.5, 0.5); nrm.module.running_var.uniform_(0.5, 2.0)
            nrm.module.weight.uniform_(0.5, 1.5); nrm.module.bias.uniform_(-0.3, 0.3)
    ora.eval()
    model = contconv.ContinuousConvModel(device="cuda", **cfg)
    _copy_state(model, ora)
    pos, vel, m = _plummer_pos(n, 1234)
    pos = pos * BENCH_SCALE_16384
    feat = torch.cat([vel, m[:, None] * n], 1)
    got = model.predict(pos.cuda(), feat.cuda()).cpu()
    assert model.last_path == ("fused", "fused")                              # the block-sparse kernels ran, not the binned fallback
    for layer in model.contconv:
        layer.use_fused = False
    slow = model.predict(pos.cuda(), feat.cuda()).cpu()
    assert model.last_path == ("binned", "binned")                            # a forced fallback shows up in last_path
    for layer in model.contconv:
        layer.use_fused = True
    assert global_rel(slow, got) < TOL

    ei = so.radius_graph(pos, 1.0, loop=True, max_num_neighbors=32)           # the oracle's own edge list
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(5))[:40]
    keep2 = torch.isin(ei[0], rows)                                           # aggregation at edge_index[0]
    need1 = torch.unique(torch.cat([rows, ei[1][keep2]]))
    keep1 = torch.isin(ei[0], need1)
    with torch.no_grad():
        x = torch.cat([pos, feat[:, 3:]], dim=1)
        enc = ora.node_encoder(x)
        h1 = torch.tanh(ora.contconv[0](pos, enc, ei[:, keep1]))              # exact on `need1`
        h2 = torch.tanh(ora.contconv[1](pos, h1, ei[:, keep2]))               # exact on `rows`
        ref = ora.output(ora.layer_norm(torch.cat((enc, h2), dim=-1)))[rows]
    assert float(h2[rows].abs().mean()) > 0.05                     # tanh in its useful range (mean |h2| ~ 0.2)
    assert global_rel(got[rows], ref) < TOL and row_rel(got[rows], ref) < 10 * TOL


def test_random_batched_graph_sweep(gpu_device):
    """30 random batches (ragged segment sizes incl. 1-node graphs, random k / radius / cap / loop): kNN and radius
    graphs index-exact against the oracle -- exercises the slice / 128-centre-group boundaries of the streaming search."""
    from nbd import graphops
    from oracle import surrogate_oracle as so
    rng = np.random.default_rng(77)
    for trial in range(30):
        n_graphs = int(rng.integers(1, 9))
        sizes = [int(rng.choice([1, 2, 3, 17, 63, 64, 65, 127, 128, 129, 200, 333])) for _ in range(n_graphs)]
        n = sum(sizes)
        pos = torch.tensor(rng.normal(size=(n, 3)) * rng.choice([0.3, 1.0, 3.0]), dtype=torch.float32)
        b = _batch(n, sizes) if n_graphs > 1 or trial % 3 else None
        k = int(rng.choice([1, 4, 10, 50, 70]))
        r = float(rng.choice([0.2, 0.7, 1.5]))
        cap = int(rng.choice([1, 5, 32, 100]))
        loop = bool(trial % 2)
        bc = b.cuda() if b is not None else None
        assert torch.equal(graphops.knn_graph(pos.cuda(), k, batch=bc).cpu(), so.knn_graph(pos, k, batch=b)), ("knn", trial)
        assert torch.equal(graphops.radius_graph(pos.cuda(), r, batch=bc, loop=loop, max_num_neighbors=cap).cpu(),
                           so.radius_graph(pos, r, batch=b, loop=loop, max_num_neighbors=cap)), ("radius", trial, sizes, r, cap)


@pytest.mark.parametrize("n", [2, 5, 51, 130])
def test_captured_gnn_step_equals_eager_for_small_systems(n, gpu_device):
    """The captured (in place, hinted kNN, packed input) step against Trainer.step for systems around the k = 50
    boundary: fewer bodies than neighbours asked for, exactly k + 1, a little more."""
    import gnn
    import trainer
    torch.manual_seed(n)
    model = gnn.GraphModel(input_dim=4, gnn_dim=32, message_passing_steps=2, aggr="mean", neighbors=10, device="cuda")
    tr = trainer.Trainer(model, None, device="cuda", dt=0.01)
    pos, vel, m = _plummer_pos(n, 40 + n)
    pos, vel, m1 = pos.cuda(), vel.cuda(), (m * n)[:, None].cuda()
    acc = model.predict(pos, torch.cat([vel, m1], 1))
    adv = tr._capture_step(pos, vel, m1, acc, 0.01)
    assert adv is not None
    p, v, a = pos, vel, acc
    for i in range(5):
        p, v, a = tr.step(p, v, m1, a, 0.01)
        gp, gv, ga = adv()
        assert torch.equal(gp, p) and torch.equal(gv, v) and torch.equal(ga, a), (n, i)


@pytest.mark.parametrize("k", [3, 0])
def test_dataset_graphs_equal_the_per_group_construction(k, tmp_path, gpu_device):
    """datautils.ParticleGraphDataset builds all graphs from one sort, one upload and one batched kNN launch. Against
    the reference's construction spelled out (datautils.py:23-48: pandas groupby (scene, step), per-group tensors,
    per-graph kNN) on a CSV whose rows are interleaved across scenes / steps, with ragged graph sizes including
    graphs of one and two nodes: same graphs in the same order, same node order, same edges."""
    import pandas as pd
    from datautils import ParticleGraphDataset
    from nbd import graphops
    rng = np.random.default_rng(21)
    rows = []
    for scene, n in ((2, 5), (0, 1), (1, 9), (3, 2)):
        mass = (rng.random(n) + 0.5).astype(np.float32)
        for step in (1, 0, 2):
            block = rng.standard_normal((n, 9)).astype(np.float32)
            rows += [[scene, step, mass[i]] + list(block[i]) for i in range(n)]
    rows = np.array(rows, dtype=np.float64)[rng.permutation(len(rows))]            # file order != group order
    path = str(tmp_path / "mixed.csv")
    _write_toy_csv(path, rows)
    ds = ParticleGraphDataset(path, k=k, device="cuda")
    df = pd.read_csv(path)
    groups = list(df.groupby(["scene", "step"]))
    assert len(ds) == len(groups) == 12
    for g, ((scene, step), grp) in zip(ds.graphs, groups):
        x = torch.tensor(grp[["x", "y", "z", "vx", "vy", "vz", "mass"]].values, dtype=torch.float)
        y = torch.tensor(grp[["ax", "ay", "az"]].values, dtype=torch.float)
        assert torch.equal(g.x.cpu(), x) and torch.equal(g.y.cpu(), y)
        assert g.scene.tolist() == [scene] * len(grp) and g.step.tolist() == [step] * len(grp)
        assert g.scene.dtype == g.step.dtype == torch.int64 and g.edge_index.dtype == torch.int64
        want = graphops.knn_graph(x[:, :3].cuda().contiguous(), k=k, loop=False) if k > 0 else \
            torch.zeros((2, 0), dtype=torch.int64, device="cuda")
        assert torch.equal(g.edge_index, want) and g.edge_index.is_contiguous()


@pytest.mark.parametrize("n,cap,loop,wide_cap", [(3000, 32, True, 128), (500, 8, False, 32), (40, 32, True, 128),
                                                  (2500, 16, True, 64)])
def test_cached_radius_search_is_exact_over_a_rollout(n, cap, loop, wide_cap, gpu_device):
    """nbd_radius_cached_search_f32 (the rollout form of the radius search: cached candidate lists within r + skin,
    re-tested every call, rebuilt when a body has moved too far) against the plain search on the same positions, step
    after step: small drifts (lists reused), then a few bodies jumping across the system (forced rebuild), with a
    dense clump whose truncated candidate lists exercise the scan-on path. Every output identical: lists, degrees,
    last index, and the transposed CSR."""
    from nbd import graphops
    rng = np.random.default_rng(n + cap)
    p = rng.standard_normal((n, 3)).astype(np.float32) * 2.0
    p[: n // 5] = p[: n // 5] * 0.05 + np.float32(0.3)                    # a clump: hundreds of bodies within r
    pos = torch.tensor(p, device="cuda")
    cache = graphops.RadiusCache(wide_cap=wide_cap)
    r = 0.7
    for step in range(14):
        got = graphops.radius_lists(pos, r, None, loop=loop, max_num_neighbors=cap, cache=cache)
        want = graphops.radius_lists(pos, r, None, loop=loop, max_num_neighbors=cap)
        assert torch.equal(got.deg, want.deg), step
        assert torch.equal(got.last, want.last), step
        mask = torch.arange(want.cap, device="cuda")[None, :] < want.deg[:, None]      # loop=False: cap + 1 slots
        assert torch.equal(got.nbr[mask], want.nbr[mask]), step
        assert torch.equal(got.rowptr, want.rowptr), step
        e = int(want.rowptr[-1])
        assert torch.equal(got.centres[:e], want.centres[:e]), step
        if step % 5 == 4:                                                  # a few bodies jump: the cache must rebuild
            idx = torch.tensor(rng.choice(n, 3, replace=False), device="cuda")
            pos[idx] = torch.tensor(rng.standard_normal((3, 3)).astype(np.float32), device="cuda")
        else:                                                              # a rollout step's drift: far below the skin
            pos = pos + torch.tensor(rng.standard_normal((n, 3)).astype(np.float32) * 2e-4, device="cuda")
    # the very same configuration again (nothing moved): still exact, and a model's predict() goes through the cache
    got = graphops.radius_lists(pos, r, None, loop=loop, max_num_neighbors=cap, cache=cache)
    want = graphops.radius_lists(pos, r, None, loop=loop, max_num_neighbors=cap)
    assert torch.equal(got.deg, want.deg) and torch.equal(got.rowptr, want.rowptr)


def test_contconv_predict_with_and_without_the_radius_cache(gpu_device):
    """ContinuousConvModel.predict over a short drifting sequence: the cached radius search changes nothing."""
    import contconv
    torch.manual_seed(3)
    model = contconv.ContinuousConvModel(in_channels=4, continuous_conv_dim=32, continuous_conv_layers=2,
                                         filter_resolution=[4, 3], radius=0.8, device="cuda").cuda().eval()
    pos, vel, m = _plummer_pos(900, 4)
    pos, vel, m = pos.cuda(), vel.cuda(), m.cuda()
    feat = torch.cat([vel, m[:, None] * 900], 1)
    for step in range(6):
        model.use_radius_cache = True
        a = model.predict(pos, feat)
        model.use_radius_cache = False
        b = model.predict(pos, feat)
        assert torch.equal(a, b), step
        pos = pos + 1e-3 * vel


def test_cached_radius_search_scans_on_behind_a_truncated_list(gpu_device):
    """A centre whose cached candidate list is truncated AND holds fewer current hits than the cap: its first
    wide_cap candidates by index all sit in the shell between r and r + skin, its real neighbours have higher indices.
    The re-test must continue with a plain scan behind the list's last index."""
    from nbd import graphops
    rng = np.random.default_rng(9)
    n, r, cap = 400, 0.7, 16
    skin = graphops.RadiusCache.SKIN * r
    d = rng.standard_normal((n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = np.zeros((n, 3), dtype=np.float32)
    p[:200] = (d[:200] * (r + 0.5 * skin)).astype(np.float32)            # shell bodies: in the wide lists, not within r
    p[200:399] = (d[200:399] * rng.uniform(0.05, 0.6, (199, 1))).astype(np.float32)
    pos = torch.tensor(p, device="cuda")                                   # body 399 sits at the origin
    cache = graphops.RadiusCache(wide_cap=64)
    for step in range(3):
        got = graphops.radius_lists(pos, r, None, loop=False, max_num_neighbors=cap, cache=cache)
        want = graphops.radius_lists(pos, r, None, loop=False, max_num_neighbors=cap)
        # (body 399 has > cap lower-indexed hits: without self loops it keeps cap + 1 of them, torch_cluster's rule)
        assert int(want.deg[399]) == cap + 1 and int(want.nbr[399, 0]) >= 200
        mask = torch.arange(want.cap, device="cuda")[None, :] < want.deg[:, None]      # loop=False: cap + 1 slots
        assert torch.equal(got.deg, want.deg) and torch.equal(got.last, want.last) and torch.equal(got.nbr[mask], want.nbr[mask])
        assert torch.equal(got.rowptr, want.rowptr)
        pos = pos + torch.tensor(rng.standard_normal((n, 3)).astype(np.float32) * 1e-4, device="cuda")


def test_cached_radius_search_over_a_real_trajectory(gpu_device):
    """600 leapfrog steps of a 4096-body Plummer sphere (the HIP integrator, dt = 0.01: bodies cross the skin many
    times, so the cache rebuilds repeatedly at its own pace): cached and plain radius search agree at every step,
    lists and transposed lists alike."""
    from galaxify import simulation
    from nbd import graphops
    from nbd.plummer import generate_plummer
    n = 4096
    p, v, m = generate_plummer(n, seed=8)
    sim = simulation.LeapFrogSimulator(positions=p * 3.0, velocities=v, masses=m, g_const=1.0, softening=0.1, dt=0.01,
                                       calc_energy=False, device="cuda")
    cache = graphops.RadiusCache()
    arange = torch.arange(32, device="cuda")[None, :]
    for step in range(600):
        sim.step()
        pos = sim.positions
        got = graphops.radius_lists(pos, 1.0, None, loop=True, max_num_neighbors=32, cache=cache)
        if step % 3 == 0:
            want = graphops.radius_lists(pos, 1.0, None, loop=True, max_num_neighbors=32)
            mask = arange < want.deg[:, None]
            e = int(want.rowptr[-1])
            ok = (torch.equal(got.deg, want.deg) and torch.equal(got.last, want.last) and torch.equal(got.nbr[mask], want.nbr[mask])
                  and torch.equal(got.rowptr, want.rowptr) and torch.equal(got.centres[:e], want.centres[:e]))
            assert ok, step
