"""GPU parity of distCUDA2 and of the MeshNet message-passing path (through the C-ABI) against the oracle and the
shim-derived golden vectors of the reference modules."""
import numpy as np
import os

import pytest

import util
from util import golden, rel_err

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from oracle import gnn_ref, raster_oracle as ro  # noqa: E402


def test_dist2_bit_exact_vs_oracle():
    from simple_knn._C import distCUDA2
    rng = np.random.default_rng(5)
    for P in (4, 100, 1023, 5000):
        pts = rng.normal(size=(P, 3)).astype(np.float32)
        if P > 20:
            pts[10] = pts[11]                      # coincident points
        got = distCUDA2(torch.tensor(pts, device="cuda")).cpu().numpy()
        np.testing.assert_array_equal(got, ro.dist2(pts))       # same fp32 association order: bit-exact
    assert distCUDA2(torch.zeros(0, 3, device="cuda")).numel() == 0


@pytest.mark.parametrize("P", [1025, 2051])
def test_dist2_brute_force_over_several_slabs_vs_oracle(P):
    """csplat_dist2 called directly (distCUDA2 takes it below 4096 points only): two and three 1024-point slabs, the last one ragged
    and with a tail that the four-wide loop leaves; every row, so a point that is the first or the last candidate of a slab too"""
    from csplat import native as n
    pts = np.random.default_rng(P).normal(size=(P, 3)).astype(np.float32)
    pts[1023] = pts[1024]                          # coincident points either side of the slab edge
    t = torch.tensor(pts, device="cuda")
    out = torch.full((P,), -7.0, dtype=torch.float32, device="cuda")
    n.check(n.lib.csplat_dist2(n.stream_handle(t.device), P, n.ptr(t), n.ptr(out)), "csplat_dist2")
    np.testing.assert_array_equal(out.cpu().numpy(), ro.dist2(pts))


def test_dist2_boxed_path_equals_brute_force_bit_for_bit():
    """csplat_dist2_ws (Morton order + bounding-box pruning, the upstream extension's scheme) against the brute-force
    kernel: identical bits on clustered, planar, duplicated and ragged inputs, and the timing that motivates it."""
    import time
    import simple_knn._C as knn
    rng = np.random.default_rng(11)
    sets = {"uniform 20001": rng.random((20001, 3)), "clusters": np.concatenate([rng.normal(c, 0.01, (3000, 3)) for c in rng.random((7, 3))]),
            "planar": np.c_[rng.random((9000, 2)), np.zeros(9000)], "line+dups": np.repeat(np.c_[np.linspace(0, 1, 2500), np.zeros((2500, 2))], 2, 0),
            "one box": rng.random((4096, 3))}
    for name, pts in sets.items():
        t = torch.tensor(pts.astype(np.float32), device="cuda")
        old = knn.BOXED_FROM
        try:
            knn.BOXED_FROM = 1 << 30
            ref = knn.distCUDA2(t)
            knn.BOXED_FROM = 1
            got = knn.distCUDA2(t)
        finally:
            knn.BOXED_FROM = old
        assert torch.equal(got, ref), name
    t = torch.tensor(rng.random((200_000, 3)).astype(np.float32), device="cuda")
    knn.distCUDA2(t); torch.cuda.synchronize()
    t0 = time.perf_counter(); got = knn.distCUDA2(t); torch.cuda.synchronize(); t_boxed = time.perf_counter() - t0
    old = knn.BOXED_FROM
    try:
        knn.BOXED_FROM = 1 << 30
        knn.distCUDA2(t); torch.cuda.synchronize()
        t0 = time.perf_counter(); ref = knn.distCUDA2(t); torch.cuda.synchronize(); t_brute = time.perf_counter() - t0
    finally:
        knn.BOXED_FROM = old
    assert torch.equal(got, ref)
    print(f"distCUDA2 P=200k: boxed {t_boxed * 1e3:.2f} ms, brute force {t_brute * 1e3:.2f} ms")
    assert t_boxed < t_brute


def test_dist2_full_size_vs_kdtree():
    """config-2 size: 100k points of synthetic scene_1 against scipy's exact kd-tree (tolerance 1e-6 rel)."""
    from scipy.spatial import cKDTree
    from simple_knn._C import distCUDA2
    from csplat import synthetic as syn
    sc = syn.scene_1(P=100_000, n_cams=1)
    pts = syn.gaussians_at(sc)["means3D"]
    got = distCUDA2(torch.tensor(pts, device="cuda")).cpu().numpy().astype(np.float64)
    dd, _ = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=4)
    ref = (dd[:, 1:] ** 2).mean(1)
    assert np.abs(got - ref).max() <= 1e-6 * ref.max() + 1e-12
    np.testing.assert_allclose(got, ref, rtol=2e-4, atol=1e-12)   # per-point: fp32 squared differences of ~1e-3 offsets


def _load(net, g, prefix):
    sd = {k[len(prefix):]: torch.tensor(g[k]) for k in g.files if k.startswith(prefix)}
    net.load_state_dict(sd)
    return net.cuda()


@pytest.mark.allow_fallbacks("shape")      # latent size 16 / 32 (the reference-run fixtures): the generic path, knowingly
def test_interaction_network_matches_reference_incl_f7():
    g = golden("gnn.npz")
    from meshnet.graph_network import InteractionNetwork
    net = _load(InteractionNetwork(16, 16, 16, 16, 2, 16), g, "inet.")
    ei = torch.tensor(g["edge_index"], device="cuda")
    x1, e1 = net(torch.tensor(g["in_x"], device="cuda"), ei, torch.tensor(g["in_e"], device="cuda"))
    assert rel_err(x1.detach().cpu().numpy(), g["in_x_out"]) < 1e-4
    np.testing.assert_array_equal(e1.detach().cpu().numpy(), g["in_e_out"])     # edge output = 2 x edge input (F7)


@pytest.mark.allow_fallbacks("shape")      # latent size 16 / 32 (the reference-run fixtures): the generic path, knowingly
def test_encode_process_decode_forward_backward_vs_reference():
    g = golden("gnn.npz")
    from meshnet.graph_network import EncodeProcessDecode
    net = _load(EncodeProcessDecode(8, 3, 4, 32, 3, 2, 32), g, "epd.")
    ei = torch.tensor(g["edge_index"], device="cuda")
    x = torch.tensor(g["epd_x"], device="cuda", requires_grad=True)
    e = torch.tensor(g["epd_e"], device="cuda", requires_grad=True)
    y = net(x, ei, e)
    assert rel_err(y.detach().cpu().numpy(), g["epd_y"]) < 1e-4                  # GNN output <= 1e-4 rel
    (y * torch.tensor(g["epd_w"], device="cuda")).sum().backward()
    assert rel_err(x.grad.cpu().numpy(), g["epd_dx"]) < 1e-4
    assert rel_err(e.grad.cpu().numpy(), g["epd_de"]) < 1e-4
    dW = net._processor.gnn_stacks[0].edge_fn[0][0].weight.grad.cpu().numpy()
    assert rel_err(dW, g["epd_dW_first"]) < 1e-4


def test_encode_process_decode_latent128_tall_graph_vs_reference():
    """The 128-wide MFMA paths held to a REFERENCE-RUN vector: gnn128.npz = the reference's EncodeProcessDecode
    (latent 128, 2 x 128 hidden, 2 message-passing steps) under the PyG shim on a graph with E = 16,640 edges -- tall enough for the
    training path's fused autograd nodes (EdgeFirstLayer / EdgeTailAggregate / csplat_dw128) -- with closed-form weights.  Rollout
    (no_grad: csplat_linear128 / csplat_gnn_node_update) and training path (forward + every kind of gradient) <= 1e-4; strict
    dispatch: nothing may leave the HIP path."""
    from csplat import native
    from meshnet.graph_network import EncodeProcessDecode
    g = golden("gnn128.npz")
    net = util.closed_form_weights(EncodeProcessDecode(8, 3, 4, 128, 2, 2, 128).to("cuda"))
    l0, l1 = net._processor.gnn_stacks
    np.testing.assert_array_equal(l0.edge_fn[0][2].weight[:2, :5].detach().cpu().numpy(), g["w_probe"])      # same weights as the generator's
    ei = torch.tensor(g["edge_index"].astype(np.int64), device="cuda")
    before = sum(native.FALLBACK_COUNTS.values())
    with torch.no_grad():
        y_eval = net(torch.tensor(g["x"], device="cuda"), ei, torch.tensor(g["e"], device="cuda"))
    assert rel_err(y_eval.cpu().numpy(), g["y_eval"]) < 1e-4
    x = torch.tensor(g["x"], device="cuda", requires_grad=True)
    e = torch.tensor(g["e"], device="cuda", requires_grad=True)
    y = net(x, ei, e)
    assert rel_err(y.detach().cpu().numpy(), g["y"]) < 1e-4
    # the fused nodes are in the graph
    names, stack, seen, keep = set(), [y.grad_fn], set(), []
    while stack:
        f = stack.pop()
        if f is None or id(f) in seen:
            continue
        keep.append(f)                       # (the wrappers of graph nodes are created on demand: hold them, or ids get recycled)
        seen.add(id(f)); names.add(type(f).__name__)
        stack += [nf for nf, _ in f.next_functions]
    assert any(n.startswith("EdgeFirstLayer") for n in names) and any(n.startswith("EdgeTailAggregate") for n in names), sorted(names)
    (y * torch.tensor(g["w"], device="cuda")).sum().backward()
    got = dict(dx=x.grad, de=e.grad, dW_edge_first0=l0.edge_fn[0][0].weight.grad, dW_edge_hidden0=l0.edge_fn[0][2].weight.grad,
               dW_edge_last1=l1.edge_fn[0][4].weight.grad, db_edge_last1=l1.edge_fn[0][4].bias.grad,
               dW_node_first1=l1.node_fn[0][0].weight.grad, dgamma_edge0=l0.edge_fn[1].weight.grad, dbeta_node1=l1.node_fn[1].bias.grad,
               dW_enc_edge=net._encoder.edge_fn[0][0].weight.grad, dW_dec_last=net._decoder.node_fn[4].weight.grad)
    # bar: 1e-4, or three times the distance of the reference's own fp32 run from the same network in fp64 (stored with the fixture:
    # ReLU pre-activations within rounding of zero make the gradients discontinuous in the rounding -- the reference's run is one
    # sample of that, ours another)
    for k, v in got.items():
        err = rel_err(v.cpu().numpy(), g[k])
        bar = max(1e-4, 3.0 * float(g["f64dist." + k]))
        assert err < bar, (k, err, bar)
    assert sum(native.FALLBACK_COUNTS.values()) == before


def test_strict_dispatch_raises_and_counts():
    """csplat.native.STRICT (set for every -m gpu test by conftest): a product function that would compose torch ops for a GPU tensor
    raises; inside allow_fallbacks() it is counted and runs"""
    from csplat import native, train as tr
    a = torch.rand(2, 3, 16, 16, device="cuda", dtype=torch.float64)
    b = torch.rand(2, 3, 16, 16, device="cuda", dtype=torch.float64)
    assert native.STRICT
    with pytest.raises(native.CsplatError, match="strict"):
        tr.l1_loss(a, b)
    n0 = native.FALLBACK_COUNTS[("train.l1_loss", "dtype")]
    with native.allow_fallbacks("dtype"):
        v = tr.l1_loss(a, b)
    assert native.FALLBACK_COUNTS[("train.l1_loss", "dtype")] == n0 + 1
    assert abs(float(v) - float((a - b).abs().mean())) < 1e-12
    assert float(tr.l1_loss(a.float(), b.float())) > 0          # the fp32 form is the HIP kernel: no report
    assert native.FALLBACK_COUNTS[("train.l1_loss", "dtype")] == n0 + 1


@pytest.mark.allow_fallbacks("shape")      # latent size 16 / 32 (the reference-run fixtures): the generic path, knowingly
def test_cloth_simulator_vs_reference():
    g = golden("gnn.npz")
    from meshnet.cloth_network import ClothMeshSimulator
    dev = "cuda"
    sim = ClothMeshSimulator(3, 8, 4, 32, 2, 2, 32, 2, 2, normalize=True, device=dev)
    sim.load_state_dict({k[4:]: torch.tensor(g[k]) for k in g.files if k.startswith("sim.") and not k.startswith("sim_")})
    sim = sim.to(dev)
    T = lambda k: torch.tensor(g[k], device=dev)  # noqa: E731
    ei = T("edge_index")
    sim.train()
    pa, ta = sim.predict_acceleration(T("sim_vel"), T("sim_type"), ei, T("epd_e"), target_velocities=T("sim_tgt"),
                                      velocity_noise=T("sim_noise"))
    assert rel_err(pa.detach().cpu().numpy(), g["sim_pred_acc"]) < 1e-4
    assert rel_err(ta.detach().cpu().numpy(), g["sim_tgt_acc"]) < 1e-4
    np.testing.assert_allclose(sim._node_normalizer._acc_sum.cpu().numpy(), g["sim_node_normalizer._acc_sum"], rtol=1e-5)
    sim.eval()
    pv = sim.predict_velocity(T("sim_vel"), T("sim_type"), ei, T("epd_e"))
    assert rel_err(pv.detach().cpu().numpy(), g["sim_pred_vel"]) < 1e-4
    sim2 = ClothMeshSimulator(3, 8, 4, 32, 2, 2, 32, 2, 2, normalize=False, device=dev)
    sim2.load_state_dict({k[5:]: torch.tensor(g[k]) for k in g.files if k.startswith("sim2.")})
    sim2 = sim2.to(dev).eval()
    assert rel_err(sim2.predict_velocity(T("sim_vel"), T("sim_type"), ei, T("epd_e")).detach().cpu().numpy(),
                   g["sim2_pred_vel"]) < 1e-4


@pytest.mark.parametrize("L,N,E", [(128, 500, 6000), (32, 64, 0), (20, 300, 2000), (6, 50, 400)])
def test_gnn_kernels_vs_numpy(L, N, E):
    """raw C-ABI kernels: CSR build, edge combine fwd/bwd, segment sum (compensated: == the fp64 sum to an ulp), row gather.
    Ragged degrees incl. isolated nodes, empty edge list, widths that are / are not multiples of 4."""
    from meshnet.graph_ops import EdgeCombine, GraphCSR, SegmentSum
    rng = np.random.default_rng(L)
    ei_np = rng.integers(0, max(N - 5, 1), size=(2, E)).astype(np.int64)      # last 5 nodes isolated
    ei = torch.tensor(ei_np, device="cuda")
    csr = GraphCSR(ei, N)
    for name, row in (("src", 0), ("dst", 1)):
        rp, pm = csr.rowptr[name].cpu().numpy(), csr.perm[name].cpu().numpy()[:E]
        np.testing.assert_array_equal(rp, np.concatenate([[0], np.cumsum(np.bincount(ei_np[row], minlength=N))]))
        np.testing.assert_array_equal(pm, np.argsort(ei_np[row], kind="stable"))   # ascending edge id inside a row
    msg = rng.normal(size=(E, L)).astype(np.float32)
    m = torch.tensor(msg, device="cuda", requires_grad=True)
    agg = SegmentSum.apply(m, csr)
    ref = np.zeros((N, L), np.float64)
    np.add.at(ref, ei_np[1], msg.astype(np.float64))
    # compensated summation in ascending edge order: the fp32 result is the fp64 sum to within an ulp, for ANY degree
    got_agg = agg.detach().cpu().numpy()
    assert np.all(np.abs(got_agg - ref) <= 1.2e-7 * np.abs(ref) + 1e-30)
    assert torch.equal(SegmentSum.apply(m, csr), agg)                         # and run-to-run identical
    gout = rng.normal(size=(N, L)).astype(np.float32)
    agg.backward(torch.tensor(gout, device="cuda"))
    np.testing.assert_array_equal(m.grad.cpu().numpy(), gout[ei_np[1]])
    xa, xb = rng.normal(size=(N, L)).astype(np.float32), rng.normal(size=(N, L)).astype(np.float32)
    ec = rng.normal(size=(E, L)).astype(np.float32)
    txa, txb, tec = (torch.tensor(a, device="cuda", requires_grad=True) for a in (xa, xb, ec))
    h = EdgeCombine.apply(txa, txb, tec, csr, True)
    href = np.maximum((xa[ei_np[1]] + xb[ei_np[0]]) + ec, 0)
    np.testing.assert_array_equal(h.detach().cpu().numpy(), href)
    gh = rng.normal(size=(E, L)).astype(np.float32)
    h.backward(torch.tensor(gh, device="cuda"))
    gm = gh * (href > 0)
    dxa = np.zeros((N, L), np.float64); np.add.at(dxa, ei_np[1], gm.astype(np.float64))
    dxb = np.zeros((N, L), np.float64); np.add.at(dxb, ei_np[0], gm.astype(np.float64))
    np.testing.assert_array_equal(tec.grad.cpu().numpy(), gm)
    assert np.all(np.abs(txa.grad.cpu().numpy() - dxa) <= 1.2e-7 * np.abs(dxa) + 1e-30)
    assert np.all(np.abs(txb.grad.cpu().numpy() - dxb) <= 1.2e-7 * np.abs(dxb) + 1e-30)


def test_config4_size_rollout_step_properties():
    """BASELINE config 4 shape (N=10k, E=300k, L=128, 15 steps): finite output, determinism (no float atomics)
    and agreement with the fp64 numpy oracle on the same weights."""
    from meshnet.cloth_network import ClothMeshSimulator
    torch.manual_seed(0)
    sim = ClothMeshSimulator(3, 8, 4, 128, 15, 2, 128, 2, 2, normalize=False, device="cuda").eval()
    N, E = 10_000, 300_000
    gen = torch.Generator().manual_seed(3)
    ei = torch.randint(0, N, (2, E), generator=gen).cuda()
    vel = (torch.randn(N, 6, generator=gen) * 0.1).cuda()
    ntype = torch.randint(0, 2, (N, 1), generator=gen).cuda()
    ef = torch.randn(E, 4, generator=gen).cuda()
    with torch.no_grad():
        a = sim.predict_velocity(vel, ntype, ei, ef)
        b = sim.predict_velocity(vel, ntype, ei, ef)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)                                                   # reproducible bit for bit
    feats = torch.cat([vel, torch.nn.functional.one_hot(ntype.squeeze().long(), 2)], 1).cpu().numpy()
    p = {k: v.detach().cpu().numpy() for k, v in sim._encode_process_decode.state_dict().items()}
    ref = vel[:, -3:].cpu().numpy() + gnn_ref.encode_process_decode(p, feats, ei.cpu().numpy(), ef.cpu().numpy())
    assert rel_err(a.cpu().numpy(), ref) < 1e-4


@pytest.mark.parametrize("M", [0, 1, 33, 4100, 70001])     # <= 65536 rows: one-tile-per-workgroup kernel; above: persistent kernel
@pytest.mark.parametrize("gather,ln", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("mode", [0, 1])
def test_linear128_vs_fp64(M, gather, ln, mode):
    """csplat_linear128 (fp32 MFMA, fused bias / gather / ReLU / LayerNorm) against fp64 torch; ragged M covers the row
    masking of the last 32-row tile.  Tolerance 1e-5 relative to the output scale (fp32 summation-order noise only)."""
    from meshnet.graph_ops import linear128
    from csplat import native as _n
    _n.check(_n.lib.csplat_linear128_mode(mode), "csplat_linear128_mode")   # 1: products through the 3-way bf16 split
    gen = torch.Generator().manual_seed(M + 7 * gather + 13 * ln)
    A = torch.randn(M, 128, generator=gen).cuda()
    W = (torch.randn(128, 128, generator=gen) * 0.1).cuda()
    b = torch.randn(128, generator=gen).cuda()
    Nn = 57
    ga, gb = torch.randn(Nn, 128, generator=gen).cuda(), torch.randn(Nn, 128, generator=gen).cuda()
    ia, ib = torch.randint(0, Nn, (M,), generator=gen).cuda(), torch.randint(0, Nn, (M,), generator=gen).cuda()
    norm = torch.nn.LayerNorm(128).cuda()
    if gather and ln and M:
        # no layer of the network has gathers AND a LayerNorm (graph_network.py:178-222: the gathers feed the first edge Linear, the
        # LayerNorm follows the last): the combination is refused, not compiled (its bf16-split instantiation spilled registers)
        with pytest.raises(_n.CsplatError, match="not combined"), torch.no_grad():
            linear128(A, W, b, alpha=4.0, relu=True, gather=(ga, ia, gb, ib), layer_norm=norm)
        return
    with torch.no_grad():
        norm.weight.copy_(torch.randn(128, generator=gen)); norm.bias.copy_(torch.randn(128, generator=gen))
        out = linear128(A, W, b, alpha=4.0, relu=True, gather=(ga, ia, gb, ib) if gather else None,
                        layer_norm=norm if ln else None)
        ref = 4.0 * (A.double() @ W.double().t()) + b.double()
        if gather:
            ref = ref + ga.double()[ia] + gb.double()[ib]
        pre = post = None
        if not gather:                                    # row-aligned addends (node-level calls)
            pre, post = torch.randn(M, 128, generator=gen).cuda(), torch.randn(M, 128, generator=gen).cuda()
            out2 = linear128(A, W, b, alpha=4.0, relu=True, layer_norm=norm if ln else None, add_pre=pre, add_post=post)
        ref = ref.relu()
        if ln:
            ref = torch.nn.functional.layer_norm(ref, (128,), norm.weight.double(), norm.bias.double(), norm.eps)
        if pre is not None and M:
            ref2 = (4.0 * (A.double() @ W.double().t()) + b.double() + pre.double()).relu()
            if ln:
                ref2 = torch.nn.functional.layer_norm(ref2, (128,), norm.weight.double(), norm.bias.double(), norm.eps)
            assert rel_err(out2.cpu().numpy(), (ref2 + post.double()).cpu().numpy()) < 1e-5
    assert out.shape == (M, 128)
    if M:
        assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 1e-5
        # in place (out aliases A) gives the same bits
        A2 = A.clone()
        with torch.no_grad():
            o2 = linear128(A2, W, b, alpha=4.0, relu=True, gather=(ga, ia, gb, ib) if gather else None,
                           layer_norm=norm if ln else None, out=A2)
        assert torch.equal(o2, out)
    _n.check(_n.lib.csplat_linear128_mode(1), "csplat_linear128_mode")       # back to the default


@pytest.mark.parametrize("M", [33, 4100, 70_001])     # node-level kernel, persistent kernel
@pytest.mark.parametrize("mode", [0, 1])
def test_linear128_weight_layouts_and_mask(M, mode):
    """csplat_linear128_ex reads column slices of a wider weight and transposes in place (no copies on the autograd path), and its
    mask epilogue is the ReLU backward of the layer whose output is handed in -- against fp64"""
    from meshnet.graph_ops import linear128, _weight_layout
    from csplat import native as _n
    _n.check(_n.lib.csplat_linear128_mode(mode), "csplat_linear128_mode")
    try:
        gen = torch.Generator().manual_seed(M + mode)
        Wf = (torch.randn(128, 384, generator=gen) * 0.2).cuda()
        Wc = (torch.randn(128, 128, generator=gen) * 0.2).cuda()
        A = torch.randn(M, 128, generator=gen).cuda()
        b = torch.randn(128, generator=gen).cuda()
        msk = torch.randn(M, 128, generator=gen).cuda()
        acc = torch.randn(M, 128, generator=gen).cuda()
        for name, W in (("slice", Wf[:, 128:256]), ("transpose", Wc.t()), ("transposed slice", Wf[:, 256:].t()), ("plain", Wc)):
            w_used, ldw, wt = _weight_layout(W)
            assert w_used.data_ptr() == W.data_ptr(), name                    # read in place
            ref = A.double() @ W.double().t() + b.double()
            got = linear128(A, W, b)
            assert rel_err(got.cpu().numpy(), ref.cpu().numpy()) < 2e-6, name
            refm = (0.5 * (A.double() @ W.double().t()) + acc.double()) * (msk > 0).double()
            gotm = linear128(A, W, None, alpha=0.5, add_post=acc, mask=msk)
            assert rel_err(gotm.cpu().numpy(), refm.cpu().numpy()) < 2e-6, name
            assert bool(((gotm == 0) | (msk > 0)).all())
            gotm2 = linear128(A, W, None, mask=msk)
            assert rel_err(gotm2.cpu().numpy(), ((A.double() @ W.double().t()) * (msk > 0).double()).cpu().numpy()) < 2e-6, name
        # the LayerNorm epilogue leaves every row's (mean, rstd) for the backward: against the separate kernel on the plain product
        from meshnet.graph_ops import _unit_ln, ln128_fwd
        unit = _unit_ln(A.device, 1e-5)
        stats = torch.empty(M, 2, device="cuda")
        xhat = linear128(A, Wc, b, layer_norm=unit, ln_stats=stats)
        xhat2, stats2 = ln128_fwd(linear128(A, Wc, b), unit.weight, unit.bias, 1e-5)
        assert rel_err(xhat.cpu().numpy(), xhat2.cpu().numpy()) < 1e-5
        assert float(((stats[:, 0] - stats2[:, 0]).abs() * stats2[:, 1]).max()) < 1e-6      # mean, in units of the row's std
        assert float(((stats[:, 1] - stats2[:, 1]).abs() / stats2[:, 1]).max()) < 1e-5      # rstd
    finally:
        _n.check(_n.lib.csplat_linear128_mode(1), "csplat_linear128_mode")


def test_rollout_inference_path_matches_autograd_path():
    """The no-grad rollout path (csplat_linear128 + carried 2^l edge scale) and the autograd path (rocBLAS GEMMs,
    EdgeCombine) are the same function: outputs within 1e-5 rel, edge output identical."""
    from meshnet.graph_network import EncodeProcessDecode, Processor
    torch.manual_seed(5)
    net = EncodeProcessDecode(8, 3, 4, 128, 4, 2, 128).cuda()
    gen = torch.Generator().manual_seed(11)
    N, E = 700, 9000
    ei = torch.randint(0, N, (2, E), generator=gen).cuda()
    x, e = torch.randn(N, 8, generator=gen).cuda(), torch.randn(E, 4, generator=gen).cuda()
    y_grad = net(x, ei, e).detach()
    with torch.no_grad():
        y_inf = net(x, ei, e)
    assert rel_err(y_inf.cpu().numpy(), y_grad.cpu().numpy()) < 1e-5
    proc = net._processor
    assert isinstance(proc, Processor)
    xl, el = torch.randn(N, 128, generator=gen).cuda(), torch.randn(E, 128, generator=gen).cuda()
    xg, eg = proc(xl, ei, el)
    with torch.no_grad():
        xi, einf = proc(xl, ei, el)
    assert torch.equal(einf, eg.detach())                       # 2^l scaling is exact in fp32
    assert rel_err(xi.cpu().numpy(), xg.detach().cpu().numpy()) < 1e-5


def test_splitk_linear_gradients_match_autograd():
    """SplitKLinear (batched split-K weight gradient) against torch autograd of F.linear, ragged tail included."""
    from meshnet.graph_ops import SplitKLinear, linear_rows
    gen = torch.Generator().manual_seed(3)
    M = 3 * SplitKLinear.CHUNK + 517
    x = torch.randn(M, 128, generator=gen).cuda().requires_grad_()
    W = (torch.randn(128, 128, generator=gen) * 0.1).cuda().requires_grad_()
    b = torch.randn(128, generator=gen).cuda().requires_grad_()
    gy = torch.randn(M, 128, generator=gen).cuda()
    for relu in (False, True):
        for t in (x, W, b):
            t.grad = None
        y = linear_rows(x, W, b, min_rows=1024, relu=relu)
        assert y.grad_fn is not None and "SplitKLinear" in type(y.grad_fn).__name__
        y.backward(gy)
        got = [t.grad.clone() for t in (x, W, b)]
        for t in (x, W, b):
            t.grad = None
        yr = torch.nn.functional.linear(x.double(), W.double(), b.double())
        yr = yr.relu() if relu else yr
        assert rel_err(y.detach().cpu().numpy(), yr.detach().cpu().numpy()) < 1e-5
        yr.backward(gy.double())
        for a, r in zip(got, (x, W, b)):
            assert rel_err(a.cpu().numpy(), r.grad.cpu().numpy()) < 1e-5
    # a width the fused kernel does not cover takes the library path inside the same Function
    x2 = torch.randn(20000, 4, generator=gen).cuda().requires_grad_()
    W2 = torch.randn(128, 4, generator=gen).cuda().requires_grad_()
    y2 = linear_rows(x2, W2, None, min_rows=1024, relu=True)
    y2.sum().backward()
    ref = (x2.detach().double() @ W2.detach().double().t())
    assert rel_err(y2.detach().cpu().numpy(), ref.relu().cpu().numpy()) < 1e-5
    assert rel_err(W2.grad.cpu().numpy(), ((ref > 0).double().t() @ x2.detach().double()).cpu().numpy()) < 1e-5


@pytest.mark.parametrize("T,R", [(1, 30000), (3, 30000), (8, 777), (2, 3), (5, 4097)])
def test_rows_dot_matches_linear_fwd_bwd(T, R):
    """csplat_rows_dot_fwd/_bwd (the simulator's 256 -> 3V output layer for T time rows) against F.linear in fp64."""
    from meshnet.graph_ops import rows_dot, RowsDot
    g = torch.Generator(device="cuda").manual_seed(T * 1000 + R)
    h = torch.randn(T, 256, device="cuda", generator=g).requires_grad_()
    W = (0.1 * torch.randn(R, 256, device="cuda", generator=g)).requires_grad_()
    b = torch.randn(R, device="cuda", generator=g).requires_grad_()
    dy = torch.randn(T, R, device="cuda", generator=g)
    y = rows_dot(h, W, b)
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith("RowsDot")      # the HIP path, not F.linear
    y.backward(dy)
    h64, W64, b64 = (t.detach().double().requires_grad_() for t in (h, W, b))
    y64 = torch.nn.functional.linear(h64, W64, b64)
    y64.backward(dy.double())
    for got, ref, name in ((y, y64, "y"), (h.grad, h64.grad, "dh"), (W.grad, W64.grad, "dW"), (b.grad, b64.grad, "db")):
        err = float((got.detach().double() - ref.detach()).abs().max() / ref.detach().abs().max().clamp_min(1e-30))
        assert err < 2e-6, (name, err)
    # deterministic: a second backward gives the same bits
    h2 = h.detach().clone().requires_grad_()
    rows_dot(h2, W.detach(), b.detach()).backward(dy)
    assert torch.equal(h2.grad, h.grad)
    # `add` (the simulator's table rows, meshnet_network.py:371): the same bits as the separate addition, gradient passed through
    base = torch.randn(T, R, device="cuda", generator=g).requires_grad_()
    ya = rows_dot(h.detach(), W.detach(), b.detach(), base)
    assert torch.equal(ya, base + y.detach())
    ya.backward(dy)
    assert torch.equal(base.grad, dy)


def test_simulator_forward_times_equals_forward_per_time_on_gpu():
    from meshnet.meshnet_network import ResidualMeshSimulator
    torch.manual_seed(3)
    mesh = torch.randn(7, 500, 3, device="cuda")
    sim = ResidualMeshSimulator(mesh, device="cuda")
    with torch.no_grad():
        sim.output.weight.mul_(1e4)          # (initialised at 1e-5: make the residual visible)
    times = [k / 6 for k in (0, 3, 4, 6)]
    both = sim.forward_times(times)
    for i, t in enumerate(times):
        one = sim(torch.tensor(t, device="cuda").repeat(500, 1))
        assert float((both[i] - one).abs().max()) < 1e-5 * float(one.abs().max())
    both.square().sum().backward()
    g_batched = sim.output.weight.grad.clone()
    sim.zero_grad()
    sum(sim(torch.tensor(t, device="cuda").repeat(500, 1)).square().sum() for t in times).backward()
    assert float((g_batched - sim.output.weight.grad).abs().max()) < 1e-4 * float(g_batched.abs().max())
    with pytest.raises(ValueError):
        sim.forward_times([0.5, 1.5])


def _irregular_graph(seed):
    """graphs unlike a cloth mesh: isolated nodes, self loops, duplicated edges, one hub collecting thousands of edges, node /
    edge counts that are multiples of nothing."""
    rng = np.random.default_rng(seed)
    N = int(rng.integers(3, 1500))
    E = int(rng.integers(0, 20000))
    src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
    if E > 50:
        k = E // 5
        dst[:k] = rng.integers(0, N)                      # hub: a fifth of the edges end in one node
        src[k:k + 10] = dst[k:k + 10]                     # self loops
        src[k + 10:k + 30], dst[k + 10:k + 30] = src[k + 30], dst[k + 30]     # 20 copies of one edge
        lonely = rng.integers(0, N, max(N // 7, 1))       # nodes without any edge
        keep = ~(np.isin(src, lonely) | np.isin(dst, lonely))
        src, dst = src[keep], dst[keep]
    return N, np.stack([src, dst]).astype(np.int64)


def _gnn_fuzz_seeds():
    import os
    lo, hi = (int(v) for v in os.environ.get("CSPLAT_GNN_FUZZ_SEEDS", "300:310").split(":"))   # (wider sweeps: 1000:1200 ...)
    return list(range(lo, hi))


@pytest.mark.parametrize("seed", _gnn_fuzz_seeds())
def test_gnn_irregular_graphs_vs_oracle(seed):
    """EncodeProcessDecode at the config-4 width (L = 128: the csplat_linear128 / node-update kernels in the no-grad path, the
    EdgeCombine / SegmentSum / split-K functions under autograd) against oracle/gnn_ref.py in fp64, forward and backward."""
    N, ei_np = _irregular_graph(seed)
    _training_path_vs_fp64(seed, N, ei_np)


def test_gnn_tall_graph_training_path_vs_oracle():
    """the same check on a graph with E >= 16384 edges: the edge-level layers take csplat_linear128 both ways, csplat_dw128, and the
    chained edge-latent gradient (graph_ops.EdgeLatentLinear) -- the functions the config-4 train step runs"""
    from meshnet.graph_ops import SplitKLinear
    rng = np.random.default_rng(77)
    N, E = 2500, 40_000
    assert E >= SplitKLinear.BIG_ROWS
    ei_np = np.stack([rng.integers(0, N, E), rng.integers(0, N, E)]).astype(np.int64)
    _training_path_vs_fp64(77, N, ei_np)


def _training_path_vs_fp64(seed, N, ei_np):
    from meshnet.graph_network import EncodeProcessDecode
    E = ei_np.shape[1]
    torch.manual_seed(seed)
    net = EncodeProcessDecode(8, 3, 4, 128, 3, 2, 128).cuda()
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 8, generator=gen).cuda().requires_grad_()
    e = torch.randn(E, 4, generator=gen).cuda().requires_grad_()
    ei = torch.tensor(ei_np, device="cuda")
    p = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    ref = gnn_ref.encode_process_decode(p, x.detach().cpu().numpy(), ei_np, e.detach().cpu().numpy())
    with torch.no_grad():
        y_inf = net(x, ei, e)
    y = net(x, ei, e)
    assert y.shape == (N, 3) and torch.isfinite(y).all()
    assert rel_err(y_inf.cpu().numpy(), ref) < 1e-4 and rel_err(y.detach().cpu().numpy(), ref) < 1e-4
    # gradients: fp64 torch restatement of the same network (PyG semantics) on the CPU -- and the same composition in plain fp32
    # torch on the GPU: a hub collecting thousands of edges makes the backward ill-conditioned in fp32 (tools/gnn_diag.py:
    # index_select / cat / index_add_ in fp32 misses the fp64 gradients by up to 1e-2 on the same graphs), so the bar is 1e-4
    # or five times what that plain fp32 composition achieves
    def composed(n_, x_, ei_, e_):
        h, ee = n_._encoder(x_, e_)
        for g_ in n_._processor.gnn_stacks:
            m = g_.edge_fn(torch.cat([h.index_select(0, ei_[1]), h.index_select(0, ei_[0]), ee], -1))
            agg = torch.zeros_like(h).index_add_(0, ei_[1], m)
            h = g_.node_fn(torch.cat([agg, h], -1)) + h
            ee = ee + ee
        return n_._decoder(h)
    w = torch.randn(N, 3, generator=gen)
    (y * w.cuda()).sum().backward()
    got = [x.grad.clone(), e.grad.clone()] + [p_.grad.clone() for p_ in net.parameters()]
    net32 = EncodeProcessDecode(8, 3, 4, 128, 3, 2, 128)                 # plain fp32 composition on the CPU: sequential
    net32.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()})   # index_add_, so this yardstick is reproducible
    x32, e32 = x.detach().cpu().requires_grad_(), e.detach().cpu().requires_grad_()
    (composed(net32, x32, torch.tensor(ei_np), e32) * w).sum().backward()
    plain = [x32.grad, e32.grad] + [p_.grad for p_ in net32.parameters()]
    net64 = EncodeProcessDecode(8, 3, 4, 128, 3, 2, 128).double()
    net64.load_state_dict({k: v.double().cpu() for k, v in net.state_dict().items()})
    x64, e64 = x.detach().cpu().double().requires_grad_(), e.detach().cpu().double().requires_grad_()
    (composed(net64, x64, torch.tensor(ei_np), e64) * w.double()).sum().backward()
    exact = [x64.grad, e64.grad] + [p_.grad for p_ in net64.parameters()]
    names = ["x", "e"] + [n_ for n_, _ in net.named_parameters()]
    errs = []
    for n_, a_, b_, c_ in zip(names, got, plain, exact):
        if c_ is None or c_.numel() == 0 or float(c_.abs().max()) == 0:
            continue
        errs.append((n_, rel_err(a_.cpu().numpy(), c_.numpy()), rel_err(b_.cpu().numpy(), c_.numpy())))
    # How accurate CAN an fp32 implementation be on this graph?  Two measurements on the EXACT (fp64) network, per graph:
    #  sens -- its gradients move by this much when every weight is perturbed by one fp32 rounding (1.2e-7 relative): a hub collecting
    #          thousands of messages makes the backward ill-conditioned (seed 305: 4e-4 on x, 1.2e-2 on e; regular graphs: 4e-7);
    #  flip -- the gradient is DISCONTINUOUS where a ReLU pre-activation crosses zero, and among ~1e6 pre-activations some lie within
    #          fp32 rounding of it (tools/gnn_layer_probe.py, seed 323: z = -4.7e-7 on a unit carrying 2.6 % of the layer's largest
    #          gradient; an fp32 forward -- any fp32 forward, the step there is two nn.Linear calls -- lands on either side).  The
    #          envelope: the fp64 gradients with every unit whose |z| < 4e-6 * (largest |z| of its row) switched on, against switched off.
    # No fp32 code path is owed more than a small multiple of either; the plain fp32 composition on the CPU is a third yardstick.
    def variant(perturb=0.0, margin=None):
        n_ = EncodeProcessDecode(8, 3, 4, 128, 3, 2, 128).double()
        gp = torch.Generator().manual_seed(seed + 1)
        n_.load_state_dict({k: v.double().cpu() * (1 + perturb * torch.randn(v.shape, generator=gp, dtype=torch.float64))
                            for k, v in net.state_dict().items()})
        if margin is not None:
            class MarginReLU(torch.nn.Module):
                def forward(self, z):
                    return z * (z > margin * z.detach().abs().amax(-1, keepdim=True)).to(z.dtype)
            def swap(m):
                for name, child in m.named_children():
                    if isinstance(child, torch.nn.ReLU):
                        setattr(m, name, MarginReLU())
                    else:
                        swap(child)
            swap(n_)
        xv, ev = x.detach().cpu().double().requires_grad_(), e.detach().cpu().double().requires_grad_()
        (composed(n_, xv, torch.tensor(ei_np), ev) * w.double()).sum().backward()
        return [xv.grad, ev.grad] + [p_.grad for p_ in n_.parameters()]

    def spread(a, b):
        return max(rel_err(m_.numpy(), c_.numpy()) for m_, c_, r_ in zip(a, b, exact)
                   if r_ is not None and r_.numel() and float(r_.abs().max()) > 0 and float(c_.abs().max()) > 0)
    sens = spread(variant(perturb=1.2e-7), exact)
    flip = spread(variant(margin=-4e-6), variant(margin=4e-6))
    for n_, eh, ep in errs:
        assert eh <= max(2e-4, 5.0 * ep, 4.0 * sens, 2.0 * flip), (n_, eh, ep, sens, flip)


@pytest.mark.allow_fallbacks("shape")      # latent size 16 / 32 (the reference-run fixtures): the generic path, knowingly
def test_edge_features_kernel_and_rollout_loop():
    """csplat_gnn_edge_features == PyG Cartesian(norm=False) + Distance(norm=False) (pos[row] - pos[col] and its norm), and
    meshnet.rollout.rollout == the reference's loop (train_meshnet_sim.py:126-265) written out in plain torch around the same
    simulator: per step features from the current positions, predict_velocity, grasp pinning, integration, history shift."""
    from meshnet.cloth_network import ClothMeshSimulator
    from meshnet.rollout import edge_features, rollout
    dev = "cuda"
    g = torch.Generator().manual_seed(12)
    N, E = 300, 2100
    pos = torch.randn(N, 3, generator=g).to(dev)
    ei = torch.randint(0, N, (2, E), generator=g).to(dev)
    ef = edge_features(pos, ei)
    d = pos.double()[ei[0]] - pos.double()[ei[1]]
    ref = torch.cat([d, d.norm(dim=1, keepdim=True)], 1)
    assert float((ef.double() - ref).abs().max()) < 1e-6
    torch.manual_seed(3)
    sim = ClothMeshSimulator(3, 8, 4, 32, 2, 2, 32, 2, 2, normalize=False, device=dev).eval()
    hist = (torch.randn(2, N, 3, generator=g) * 0.01).to(dev)
    ntype = torch.randint(0, 2, (N, 1), generator=g).to(dev)
    actions = (torch.randn(4, 3, generator=g) * 0.01).to(dev)
    preds, pos_end = rollout(sim, pos, hist, ntype, ei, actions, 7, 4)
    with torch.no_grad():
        p, h, outs = pos.clone(), hist.clone(), []
        for step in range(4):
            dd = p[ei[0]] - p[ei[1]]
            feats = torch.cat([dd, dd.norm(dim=1, keepdim=True)], 1)
            v = sim.predict_velocity(torch.cat([h[0], h[1]], 1), ntype, ei, feats)
            v[7] = actions[step]
            outs.append(v); p = p + v
            h = torch.stack([h[1], v])
    assert rel_err(preds.cpu().numpy(), torch.stack(outs).cpu().numpy()) < 1e-5
    assert rel_err(pos_end.cpu().numpy(), p.cpu().numpy()) < 1e-5
    assert torch.equal(preds[:, 7], actions)


def test_real_world_edge_length_refinement_kernel_and_rollout():
    """csplat_gnn_edge_length_refine (one launch per Adam iteration, node-centric, no autograd) against the reference's own `real_world`
    branch (train_meshnet_sim.py:212-250, its text exec'd by tests/golden/make_golden.py: refine.npz) and against the same optimisation in
    fp64; then meshnet.rollout.rollout(real_world=True) against the loop written out in plain torch with the host form of the refinement
    (which tests/test_oracle_cpu.py holds to the same fixture).  Degenerate inputs: a zero-length edge, a self loop, an isolated node."""
    from meshnet.cloth_network import ClothMeshSimulator
    from meshnet.rollout import refine_edge_lengths, rollout
    dev = "cuda"
    d = util.golden("refine.npz")
    for name in ("a", "b"):
        t = lambda k: torch.from_numpy(d[f"{name}.{k}"])  # noqa: E731
        grasped = int(d[f"{name}.grasped"])
        v = refine_edge_lengths(t("pos").to(dev), t("v").to(dev), t("edge_index").to(dev), t("rest_len").to(dev), grasped)
        again = refine_edge_lengths(t("pos").to(dev), t("v").to(dev), t("edge_index").to(dev), t("rest_len").to(dev), grasped)
        assert torch.equal(v, again)                                  # no atomics: the same bits
        v[grasped] = t("action").to(dev)
        ref = t("v_refined")
        assert float((v.cpu() - ref).abs().max()) <= 2e-6 * float(ref.abs().max()), name
        v64 = refine_edge_lengths(t("pos").double(), t("v").double(), t("edge_index"), t("rest_len").double(), grasped)
        v64[grasped] = t("action").double()
        assert float((v.cpu().double() - v64).abs().max()) <= 2e-6 * float(v64.abs().max()), name
    # degenerate edges: (3 -> 3) self loop, an edge whose ends coincide (len 0: torch.norm's backward is 0 there), node 9 isolated
    g = torch.Generator().manual_seed(5)
    N = 10
    pos = torch.randn(N, 3, generator=g) * 0.1
    pos[6] = pos[5]
    v0 = torch.zeros(N, 3)
    ei = torch.tensor([[0, 1, 3, 5, 2, 4, 7, 8], [1, 2, 3, 6, 0, 7, 8, 4]])
    rl = torch.rand(ei.shape[1], generator=g) * 0.1
    out = refine_edge_lengths(pos.to(dev), v0.to(dev), ei.to(dev), rl.to(dev), None)
    ref = refine_edge_lengths(pos.double(), v0.double(), ei, rl.double(), None)
    assert torch.isfinite(out).all() and float((out.cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert float(out[9].abs().max()) == 0.0
    # the rollout loop with real_world=True
    N, E = 300, 2100
    pos = torch.randn(N, 3, generator=g).to(dev)
    ei = torch.randint(0, N, (2, E), generator=g).to(dev)
    torch.manual_seed(3)
    sim = ClothMeshSimulator(3, 8, 4, 128, 2, 2, 128, 2, 2, normalize=False, device=dev).eval()
    hist = (torch.randn(2, N, 3, generator=g) * 0.01).to(dev)
    ntype = torch.randint(0, 2, (N, 1), generator=g).to(dev)
    actions = (torch.randn(3, 3, generator=g) * 0.01).to(dev)
    preds, pos_end = rollout(sim, pos, hist, ntype, ei, actions, 7, 3, real_world=True)
    L0 = torch.norm(pos[ei[1]] - pos[ei[0]], dim=1)
    with torch.no_grad():
        p, h, outs = pos.clone(), hist.clone(), []
        for step in range(3):
            dd = p[ei[0]] - p[ei[1]]
            feats = torch.cat([dd, dd.norm(dim=1, keepdim=True)], 1)
            v = sim.predict_velocity(torch.cat([h[0], h[1]], 1), ntype, ei, feats)
            v = refine_edge_lengths(p.cpu().double(), v.cpu().double(), ei.cpu(), L0.cpu().double(), 7).float().to(dev)
            v[7] = actions[step]
            outs.append(v); p = p + v
            h = torch.stack([h[1], v])
    assert rel_err(preds.cpu().numpy(), torch.stack(outs).cpu().numpy()) < 1e-4
    assert rel_err(pos_end.cpu().numpy(), p.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("mode", [0, 1])
def test_linear128_wide_dynamic_range_rows(mode):
    """rows whose entries span many orders of magnitude (1e-6 .. 1e+4 inside a row, denormal-adjacent and huge rows side by side),
    against fp64, error relative to each ROW's own output scale (not the matrix's): <= 1e-5.  At M = 4096 and without a gather
    csplat_linear128_ex takes k_linear128_rows32 (ntile <= 2048), which is fp32 MFMA only and does not look at the product mode: both
    parameters run that kernel.  The 3-way bf16 split -- three pieces that share ONE exponent range per value, where a split scheme
    would lose small terms if pieces were dropped -- is given these rows, per row and per row class, at the persistent sizes by
    tests/test_gnn_kernels_gpu.py::test_linear128_persistent_row_classes_every_epilogue and
    ::test_linear128_gather_every_size_and_index_pattern.  """
    from meshnet.graph_ops import linear128
    from csplat import native as _n
    _n.check(_n.lib.csplat_linear128_mode(mode), "csplat_linear128_mode")
    try:
        gen = torch.Generator().manual_seed(99)
        M = 4096
        mag = 10.0 ** (torch.rand(M, 128, generator=gen) * 10.0 - 6.0)                     # 1e-6 .. 1e+4 within a row
        A = (torch.randn(M, 128, generator=gen) * mag)
        A[:64] *= 1e-30                                                                     # tiny rows (products near 1e-36)
        A[64:128] *= 1e+20                                                                  # huge rows
        A[128:192] = 0.0
        A[128:192, 5] = 1e-3                                                                # one-hot-ish rows
        W = torch.randn(128, 128, generator=gen) * 10.0 ** (torch.rand(128, 128, generator=gen) * 6.0 - 3.0)
        b = torch.zeros(128)
        with torch.no_grad():
            out = linear128(A.cuda(), W.cuda(), b.cuda()).cpu().double()
        ref = A.double() @ W.double().t()
        # fp32 accumulation bound: error <= ~K * eps * sum_k |a_k w_k| per output; compare against that magnitude row-wise
        bound = (A.double().abs() @ W.double().abs().t()).amax(dim=1, keepdim=True) + 1e-300
        err = ((out - ref).abs() / bound).max().item()
        assert err < 1e-5, err
        assert torch.isfinite(out).all()
    finally:
        _n.check(_n.lib.csplat_linear128_mode(1), "csplat_linear128_mode")


@pytest.mark.parametrize("M", [1, 7, 300, 70_001])
def test_layernorm128_and_relu_mask_bias_vs_fp64(M):
    """csplat_ln128_fwd / _bwd against torch.nn.functional.layer_norm in fp64 (value 1e-6, gradients 1e-5 relative), run to run
    bit-identical gamma / beta gradients; csplat_relu_mask_bias128 against threshold_backward + sum(0)."""
    from meshnet.graph_ops import LayerNorm128, relu_mask_bias128
    gen = torch.Generator().manual_seed(M)
    x = (torch.randn(M, 128, generator=gen) * 3 + 0.5).cuda().requires_grad_(True)
    ga = torch.randn(128, generator=gen).cuda().requires_grad_(True)
    be = torch.randn(128, generator=gen).cuda().requires_grad_(True)
    w = torch.randn(M, 128, generator=gen).cuda()
    y = LayerNorm128.apply(x, ga, be, 1e-5)
    (y * w).sum().backward()
    x64, g64, b64 = (t.detach().double().requires_grad_(True) for t in (x, ga, be))
    y64 = torch.nn.functional.layer_norm(x64, (128,), g64, b64, 1e-5)
    (y64 * w.double()).sum().backward()
    assert rel_err(y.detach().cpu().numpy(), y64.detach().cpu().numpy()) < 2e-6
    assert rel_err(x.grad.cpu().numpy(), x64.grad.cpu().numpy()) < 1e-5
    assert rel_err(ga.grad.cpu().numpy(), g64.grad.cpu().numpy()) < 1e-5
    assert rel_err(be.grad.cpu().numpy(), b64.grad.cpu().numpy()) < 1e-5
    first = (ga.grad.clone(), be.grad.clone())
    x.grad = ga.grad = be.grad = None
    (LayerNorm128.apply(x, ga, be, 1e-5) * w).sum().backward()
    assert torch.equal(ga.grad, first[0]) and torch.equal(be.grad, first[1])
    out = torch.randn(M, 128, generator=gen).cuda()
    gm, db = relu_mask_bias128(w, out)
    ref = torch.ops.aten.threshold_backward(w, out, 0)
    assert torch.equal(gm, ref)
    assert rel_err(db.cpu().numpy(), ref.double().sum(0).cpu().numpy()) < 1e-5
    g2, db2 = relu_mask_bias128(w, None)
    assert g2.data_ptr() == w.data_ptr() and rel_err(db2.cpu().numpy(), w.double().sum(0).cpu().numpy()) < 1e-5
    # the two extras of csplat_ln128_bwd the fused message path uses: column sums of dx, and the incoming gradient read through a
    # row index (the backward of the segmented sum behind the LayerNorm)
    from meshnet.graph_ops import ln128_bwd, ln128_fwd
    xd = x.detach()
    _, stats = ln128_fwd(xd, ga.detach(), be.detach(), 1e-5)
    dx, dga, dbe, dxs = ln128_bwd(w, xd, stats, ga.detach(), want_dxsum=True)
    assert torch.equal(dx, x.grad) and torch.equal(dga, first[0]) and torch.equal(dbe, first[1])
    assert float((dxs.double() - dx.double().sum(0)).abs().max()) <= 1e-5 * float(dx.double().abs().sum(0).max()) + 1e-12
    R = max(M // 3, 1)
    rows = torch.randint(0, R, (M,), generator=gen).cuda()
    small = torch.randn(R, 128, generator=gen).cuda()
    dxg, dgg, dbg, _ = ln128_bwd(small, xd, stats, ga.detach(), g_rows=rows)
    dxr, dgr, dbr, _ = ln128_bwd(small[rows].contiguous(), xd, stats, ga.detach())
    assert torch.equal(dxg, dxr) and torch.equal(dgg, dgr) and torch.equal(dbg, dbr)


@pytest.mark.parametrize("M", [1, 2, 3, 31, 63, 64, 65, 127, 1000, 10_000, 16_385, 70_001, 300_000])
def test_dw128_vs_fp64(M):
    """csplat_dw128 (g^T x on fp32 MFMA, deterministic split-K) against fp64: error relative to sum |g||x| per output <= 2e-6
    (fp32 accumulation over up to 3e5 rows), twice the same bits."""
    from meshnet.graph_ops import dw128
    gen = torch.Generator().manual_seed(M)
    g = torch.randn(M, 128, generator=gen).cuda()
    x = (torch.randn(M, 128, generator=gen) * 2 + 0.3).cuda()
    dW = dw128(g, x)
    ref = g.double().t() @ x.double()
    bound = (g.double().abs().t() @ x.double().abs()).clamp_min(1e-30)
    assert float(((dW.double() - ref).abs() / bound).max()) < 2e-6
    assert torch.equal(dW, dw128(g, x))
    # bias gradient from the same pass; max(x, 0) as the second operand
    dW2, db = dw128(g, x, bias=True)
    assert torch.equal(dW2, dW)
    assert float(((db.double() - g.double().sum(0)).abs() / g.double().abs().sum(0).clamp_min(1e-30)).max()) < 2e-6
    dW3, db3 = dw128(g, x, bias=True, x_relu=True)
    assert torch.equal(db3, db) and torch.equal(dW3, dw128(g, x.relu()))
    assert torch.equal(dw128(g, x, x_relu=True), dW3)


@pytest.mark.parametrize("T", [1, 3, 8])
def test_sim_hidden_layers_match_composed_torch_fwd_bwd(T):
    """csplat_sim_hidden_fwd / _bwd (relu(Linear(13, 256)) -> relu(Linear(256, 256)) of the time-conditioned simulator,
    meshnet_network.py:337-338,364-366, one launch each way) against the same two layers composed in fp64: output and the four
    parameter gradients; the node is the one the simulator's _residual() takes on the GPU."""
    from meshnet.graph_ops import sim_hidden
    g = torch.Generator().manual_seed(40 + T)
    lin1, lin2 = torch.nn.Linear(13, 256), torch.nn.Linear(256, 256)
    with torch.no_grad():
        lin1.bias.add_(0.3 * torch.randn(256, generator=g)); lin2.bias.add_(0.3 * torch.randn(256, generator=g))
    e = torch.randn(T, 13, generator=g)
    w = torch.randn(T, 256, generator=g)
    d1, d2 = torch.nn.Linear(13, 256).double(), torch.nn.Linear(256, 256).double()
    d1.load_state_dict({k: v.double() for k, v in lin1.state_dict().items()}); d2.load_state_dict({k: v.double() for k, v in lin2.state_dict().items()})
    ref = torch.relu(d2(torch.relu(d1(e.double()))))
    (ref * w.double()).sum().backward()
    lin1, lin2 = lin1.cuda(), lin2.cuda()
    out = sim_hidden(e.cuda(), lin1, lin2)
    assert type(out.grad_fn).__name__.startswith("SimHidden")
    (out * w.cuda()).sum().backward()
    assert rel_err(out.detach().cpu().numpy(), ref.detach().numpy()) < 1e-5
    for a, b in ((lin1.weight, d1.weight), (lin1.bias, d1.bias), (lin2.weight, d2.weight), (lin2.bias, d2.bias)):
        assert rel_err(a.grad.cpu().numpy(), b.grad.numpy()) < 1e-5
    # the one-node form of the whole residual MLP (SimResidual = these two layers + the 256 -> 3V output layer + the table rows): the same
    # bits as the two nodes chained
    from meshnet.graph_ops import rows_dot, sim_residual
    lo = torch.nn.Linear(256, 3 * 211).cuda()
    base = torch.randn(T, 3 * 211, device="cuda", generator=torch.Generator(device="cuda").manual_seed(T)).requires_grad_()
    wy = torch.randn(T, 3 * 211, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9 + T))
    params = list(lin1.parameters()) + list(lin2.parameters()) + list(lo.parameters())
    for p_ in params:
        p_.grad = None
    y2 = rows_dot(sim_hidden(e.cuda(), lin1, lin2), lo.weight, lo.bias, base)
    (y2 * wy).sum().backward()
    two = [p_.grad.clone() for p_ in params] + [base.grad.clone()]
    for p_ in params + [base]:
        p_.grad = None
    y1 = sim_residual(e.cuda(), lin1, lin2, lo, base)
    assert type(y1.grad_fn).__name__.startswith("SimResidual") and torch.equal(y1, y2)
    (y1 * wy).sum().backward()
    for a, b in zip([p_.grad for p_ in params] + [base.grad], two):
        assert torch.equal(a, b)


@pytest.mark.parametrize("E", [1, 31, 257, 4100, 70_001])       # ragged: the last 32-row tile is partial, odd and even tile counts per workgroup
@pytest.mark.parametrize("alpha", [1.0, 8.0, 16384.0])           # 2^l, l = 0 .. 14 on the 15-layer network
@pytest.mark.parametrize("mode", [0, 1])                         # two fp16 pieces (default) / three bf16 pieces per operand
def test_edge_mlp3_one_launch_vs_fp64_and_vs_three_launches(E, alpha, mode):
    """csplat_gnn_edge_mlp3 (the whole message MLP of an InteractionNetwork layer in one launch: gathers + three 128 x 128 layers +
    LayerNorm, inner activations in registers; /root/reference/meshnet/graph_network.py:178-199) against the fp64 composition
    (1e-5 of the output scale -- the bar of csplat_linear128) and against the three csplat_linear128 launches it replaces (same
    products on the same matrix cores in another order: 1e-5).  e0 is scaled so that alpha * e0 stays O(1), as the network's
    LayerNorm'd edge latents do."""
    from meshnet.graph_ops import edge_mlp3, edge_mlp3_mode, edge_mlp3_pack, linear128
    gen = torch.Generator().manual_seed(E + int(alpha))
    Nn = 91
    e0 = (torch.randn(E, 128, generator=gen) / alpha).cuda()
    W = [(torch.randn(128, 128, generator=gen) * 0.12).cuda() for _ in range(3)]
    b = [torch.randn(128, generator=gen).cuda() * 0.3 for _ in range(3)]
    xa, xb = torch.randn(Nn, 128, generator=gen).cuda(), torch.randn(Nn, 128, generator=gen).cuda()
    ia, ib = torch.randint(0, Nn, (E,), generator=gen).cuda(), torch.randint(0, Nn, (E,), generator=gen).cuda()
    norm = torch.nn.LayerNorm(128).cuda()
    wide = torch.randn(128, 384, generator=gen).cuda() * 0.12         # W0 as a column slice of the wider first-layer weight (ld = 384)
    W0 = wide[:, 256:]
    with torch.no_grad():
        norm.weight.copy_(torch.randn(128, generator=gen)); norm.bias.copy_(torch.randn(128, generator=gen))
        was = edge_mlp3_mode(mode)
        try:
            img = edge_mlp3_pack(W0, W[1], W[2])
            out = edge_mlp3(e0, alpha, xa, ia, xb, ib, img, b[0], b[1], b[2], norm)
        finally:
            edge_mlp3_mode(was)
        h = (alpha * (e0.double() @ W0.double().t()) + b[0].double() + xa.double()[ia] + xb.double()[ib]).relu()
        h = (h @ W[1].double().t() + b[1].double()).relu()
        h = h @ W[2].double().t() + b[2].double()
        ref = torch.nn.functional.layer_norm(h, (128,), norm.weight.double(), norm.bias.double(), norm.eps)
        t = linear128(e0, W0, b[0], alpha=alpha, relu=True, gather=(xa, ia, xb, ib))
        t = linear128(t, W[1], b[1], relu=True)
        three = linear128(t, W[2], b[2], layer_norm=norm)
    assert out.shape == (E, 128) and torch.isfinite(out).all()
    assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 1e-5
    assert rel_err(out.cpu().numpy(), three.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("N", [1, 33, 10_000])
@pytest.mark.parametrize("has_next", [False, True])
@pytest.mark.parametrize("mode,mag", [(0, 1.0), (0, 1e-2), (0, 300.0), (1, 1.0)])
def test_node_update_packed_vs_fp64_and_vs_exact_kernel(N, has_next, mode, mag):
    """csplat_gnn_node_update_packed (pre-packed weights, two fp16 pieces per operand at a fixed 2^-4 scale -- mode 0 -- or three bf16 pieces
    -- mode 1; /root/reference/meshnet/graph_network.py:203-222) against the fp64 composition and against csplat_gnn_node_update (exact
    fp32 MFMA): 1e-5 of each output's scale; aggregates of O(30) and latents of O(5) as the rollout has them, and 100 times less / 300
    times more for the fp16 mode's range."""
    from meshnet.graph_ops import edge_mlp3_mode, node_update, node_update_pack, node_update_packed
    gen = torch.Generator().manual_seed(N + has_next)
    agg, x = (torch.randn(N, 128, generator=gen) * 30 * mag).cuda(), (torch.randn(N, 128, generator=gen) * 5 * mag).cuda()
    was = edge_mlp3_mode(mode)
    W = [(torch.randn(128, 128, generator=gen) * 0.1).cuda() for _ in range(6)]
    b = [torch.randn(128, generator=gen).cuda() * 0.3 for _ in range(3)]
    l2, l3 = torch.nn.Linear(128, 128).cuda(), torch.nn.Linear(128, 128).cuda()
    norm = torch.nn.LayerNorm(128).cuda()
    with torch.no_grad():
        l2.weight.copy_(W[2]); l2.bias.copy_(b[1]); l3.weight.copy_(W[3]); l3.bias.copy_(b[2])
        norm.weight.copy_(torch.randn(128, generator=gen)); norm.bias.copy_(torch.randn(128, generator=gen))
        wi, wj = (W[4], W[5]) if has_next else (None, None)
        img = node_update_pack(W[0], W[1], W[2], W[3], wi, wj)
        got = node_update_packed(agg, x, img, b[0], b[1], b[2], norm, has_next)
        exact = node_update(agg, x, W[0], W[1], b[0], l2, l3, norm, wi, wj)
        h = (agg.double() @ W[0].double().t() + x.double() @ W[1].double().t() + b[0].double()).relu()
        h = (h @ W[2].double().t() + b[1].double()).relu()
        xn = torch.nn.functional.layer_norm(h @ W[3].double().t() + b[2].double(), (128,), norm.weight.double(), norm.bias.double(), norm.eps) + x.double()
        ref = [xn, xn @ W[4].double().t(), xn @ W[5].double().t()] if has_next else [xn, None, None]
    for g, e, r in zip(got, exact, ref):
        if r is None:
            assert g is None
            continue
        assert rel_err(g.cpu().numpy(), r.cpu().numpy()) < 1e-5 and rel_err(g.cpu().numpy(), e.cpu().numpy()) < 1e-5
    # the aggregate handed over as pieces (0 .. 4 per node, in order): bit-equal to the same launch on their sums
    cnt = torch.randint(0, 5, (N,), generator=gen)
    pp = torch.zeros(N + 1, dtype=torch.int32); pp[1:] = torch.cumsum(cnt, 0).to(torch.int32)
    pieces = (torch.randn(int(pp[-1]) + 1, 128, generator=gen) * 10).cuda()
    agg2 = torch.zeros(N, 128, device="cuda")
    for j in range(4):                                           # the same order of addition as the kernel's loop
        sel = (cnt > j).cuda()
        agg2[sel] = agg2[sel] + pieces[(pp[:-1].long() + j).cuda()[sel]]
    with torch.no_grad():
        a = node_update_packed(pieces, x, img, b[0], b[1], b[2], norm, has_next, piece_ptr=pp.cuda())
        c = node_update_packed(agg2, x, img, b[0], b[1], b[2], norm, has_next)
    edge_mlp3_mode(was)
    for u, v_ in zip(a, c):
        assert (u is None and v_ is None) or torch.equal(u, v_)


@pytest.mark.parametrize("E,N", [(5, 3), (1000, 7), (20_011, 900), (70_001, 40_000)])
def test_edge_mlp3_fused_aggregation_vs_messages_and_segment_sum(E, N):
    """csplat_gnn_edge_mlp3 with `pieces` (the launch sums its messages over runs of equal destination, cut every 8 rows; a node's
    aggregate = csplat_gnn_segment_sum over its consecutive pieces) against the same launch writing the E message rows + the segmented
    sum over them: the same per-node sums (/root/reference/meshnet/graph_network.py:201-222, aggr = 'add') to fp32 rounding of another
    order of addition, zero rows for nodes without edges, deterministic.  Graphs: a hub with hundreds of edges (runs across many 8-row
    groups and tiles), many nodes without edges, E not a multiple of 8 or 32."""
    from meshnet.graph_ops import GraphCSR, SegmentSum, absmax, edge_mlp3, edge_mlp3_pack, gather_rows, segment_sum_rows
    gen = torch.Generator().manual_seed(E)
    dst = torch.randint(0, N, (E,), generator=gen)
    dst[: E // 3] = N // 2                                   # a hub
    src = torch.randint(0, N, (E,), generator=gen)
    ei = torch.stack([src, dst]).cuda()
    e0 = torch.randn(E, 128, generator=gen).cuda()
    W = [(torch.randn(128, 128, generator=gen) * 0.1).cuda() for _ in range(3)]
    b = [torch.randn(128, generator=gen).cuda() * 0.3 for _ in range(3)]
    xa, xb = torch.randn(N, 128, generator=gen).cuda(), torch.randn(N, 128, generator=gen).cuda()
    norm = torch.nn.LayerNorm(128).cuda()
    with torch.no_grad():
        csr = GraphCSR(ei, N)
        plan = csr.agg_plan()
        assert plan["npieces"] <= E // 8 + 1 + N and int(plan["pp"][-1]) == plan["npieces"]
        img, am = edge_mlp3_pack(*W), absmax(e0)
        msg = edge_mlp3(e0, 2.0, xa, ei[1], xb, ei[0], img, b[0], b[1], b[2], norm, e0_absmax=am)
        ref = SegmentSum.apply(msg, csr)
        runs = []
        for _ in range(2):
            pieces = torch.full((plan["npieces"], 128), float("nan"), device="cuda")
            edge_mlp3(gather_rows(e0, plan["perm"]), 2.0, xa, plan["dst"], xb, plan["src"], img, b[0], b[1], b[2], norm, e0_absmax=am,
                      agg=(plan["gp0"], pieces))
            assert torch.isfinite(pieces).all()              # every piece has a writer
            runs.append(segment_sum_rows(pieces, plan["pp"], plan["iota"], N))
    assert torch.equal(runs[0], runs[1])
    assert rel_err(runs[0].cpu().numpy(), ref.cpu().numpy()) < 2e-6
    empty = torch.bincount(dst, minlength=N) == 0
    assert float(runs[0][empty.cuda()].abs().max() if empty.any() else 0.0) == 0.0


def test_edge_mlp3_fp16_overflow_is_visible_and_bf16_mode_is_not_affected():
    """The documented failure mode of the fp16-piece arithmetic (include/csplat.h): inner activations far above the
    edge rows' scale (here a first-layer weight of 3e4: ~1e6 times the inputs) leave fp16's range and the rows come out non-finite --
    visible, never a silently wrong finite row -- while mode 1 (three bf16 pieces, fp32's exponent range) still matches fp64."""
    from meshnet.graph_ops import edge_mlp3, edge_mlp3_mode, edge_mlp3_pack
    gen = torch.Generator().manual_seed(11)
    E, Nn = 4100, 50
    e0 = torch.randn(E, 128, generator=gen).cuda()
    W = [(torch.randn(128, 128, generator=gen) * s_).cuda() for s_ in (3e4, 0.1, 0.1)]
    b = [torch.randn(128, generator=gen).cuda() * 0.3 for _ in range(3)]
    xa, xb = torch.randn(Nn, 128, generator=gen).cuda(), torch.randn(Nn, 128, generator=gen).cuda()
    ia, ib = torch.randint(0, Nn, (E,), generator=gen).cuda(), torch.randint(0, Nn, (E,), generator=gen).cuda()
    norm = torch.nn.LayerNorm(128).cuda()
    with torch.no_grad():
        h = (e0.double() @ W[0].double().t() + b[0].double() + xa.double()[ia] + xb.double()[ib]).relu()
        h = (h @ W[1].double().t() + b[1].double()).relu()
        ref = torch.nn.functional.layer_norm(h @ W[2].double().t() + b[2].double(), (128,), norm.weight.double(), norm.bias.double(), norm.eps)
        outs = {}
        for mode in (0, 1):
            was = edge_mlp3_mode(mode)
            try:
                outs[mode] = edge_mlp3(e0, 1.0, xa, ia, xb, ib, edge_mlp3_pack(*W), b[0], b[1], b[2], norm)
            finally:
                edge_mlp3_mode(was)
    assert not torch.isfinite(outs[0]).all()
    bad = ~torch.isfinite(outs[0]).all(1)
    good = ~bad
    if good.any():                                  # whatever row stayed in range is right
        assert rel_err(outs[0][good].cpu().numpy(), ref[good].cpu().numpy()) < 1e-4
    assert torch.isfinite(outs[1]).all() and rel_err(outs[1].cpu().numpy(), ref.cpu().numpy()) < 1e-5


def test_edge_mlp3_row_chunks():
    """csplat_gnn_edge_mlp3 addresses its rows through 32-bit buffer offsets and therefore walks edge lists longer than 2^22 rows in chunks
    (index arrays, piece numbering and outputs offset per chunk).  With CSPLAT_EM_CHUNK_ROWS=4096 in a fresh process, E = 10,005 takes
    three launches: messages and fused aggregation bit-equal to the one-launch results."""
    import subprocess
    import sys
    code = r"""
import os, sys, torch
sys.path.insert(0, os.path.join(os.getcwd(), "cloth-splatting_amd"))
from meshnet.graph_ops import GraphCSR, absmax, edge_mlp3, edge_mlp3_pack, gather_rows
gen = torch.Generator().manual_seed(3)
E, N = 10_005, 300
ei = torch.stack([torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)]).cuda()
e0 = torch.randn(E, 128, generator=gen).cuda()
W = [(torch.randn(128, 128, generator=gen) * 0.1).cuda() for _ in range(3)]
b = [torch.randn(128, generator=gen).cuda() * 0.3 for _ in range(3)]
xa, xb = torch.randn(N, 128, generator=gen).cuda(), torch.randn(N, 128, generator=gen).cuda()
norm = torch.nn.LayerNorm(128).cuda()
with torch.no_grad():
    plan = GraphCSR(ei, N).agg_plan()
    img, am = edge_mlp3_pack(*W), absmax(e0)
    msg = edge_mlp3(e0, 4.0, xa, ei[1], xb, ei[0], img, b[0], b[1], b[2], norm, e0_absmax=am)
    pieces = torch.zeros(plan["npieces"], 128, device="cuda")
    edge_mlp3(gather_rows(e0, plan["perm"]), 4.0, xa, plan["dst"], xb, plan["src"], img, b[0], b[1], b[2], norm, e0_absmax=am, agg=(plan["gp0"], pieces))
torch.save({"msg": msg.cpu(), "pieces": pieces.cpu()}, sys.argv[1])
"""
    import tempfile
    outs = []
    with tempfile.TemporaryDirectory() as td:
        for chunk in ("", "4096"):
            path = os.path.join(td, f"o{chunk}.pt")
            env = dict(os.environ)
            env.pop("CSPLAT_EM_CHUNK_ROWS", None)
            if chunk:
                env["CSPLAT_EM_CHUNK_ROWS"] = chunk
            subprocess.run([sys.executable, "-c", code, path], check=True, env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            outs.append(torch.load(path))
    assert torch.equal(outs[0]["msg"], outs[1]["msg"]) and torch.equal(outs[0]["pieces"], outs[1]["pieces"])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scale", [1.0, 1e-3, 300.0])
def test_edge_mlp3_network_magnitudes(mode, scale):
    """What the rollout really feeds csplat_gnn_edge_mlp3: LayerNorm'd edge latents of O(1) -- here also 1e-3 and 300 times that -- under
    alpha = 2^l up to 16384, so that layer 1's pre-activations reach 1e4-1e6 before the final LayerNorm brings them back.  Mode 0 keeps its
    fp16 pieces in range by the power of two it takes from max |e0| (csplat_absmax); both modes hold 1e-5 of the output scale against
    the fp64 composition."""
    from meshnet.graph_ops import absmax, edge_mlp3, edge_mlp3_mode, edge_mlp3_pack
    E, Nn = 20_001, 700
    for alpha in (1.0, 64.0, 16384.0):
        gen = torch.Generator().manual_seed(int(alpha) + mode)
        e0 = (torch.randn(E, 128, generator=gen) * scale).cuda()
        W = [(torch.randn(128, 128, generator=gen) * 0.1).cuda() for _ in range(3)]
        b = [torch.randn(128, generator=gen).cuda() * 0.3 for _ in range(3)]
        xa, xb = torch.randn(Nn, 128, generator=gen).cuda() * 2, torch.randn(Nn, 128, generator=gen).cuda() * 2
        ia, ib = torch.randint(0, Nn, (E,), generator=gen).cuda(), torch.randint(0, Nn, (E,), generator=gen).cuda()
        norm = torch.nn.LayerNorm(128).cuda()
        with torch.no_grad():
            am = absmax(e0)
            assert float(am) == float(e0.abs().max())
            was = edge_mlp3_mode(mode)
            try:
                out = edge_mlp3(e0, alpha, xa, ia, xb, ib, edge_mlp3_pack(*W), b[0], b[1], b[2], norm, e0_absmax=am)
            finally:
                edge_mlp3_mode(was)
            h = (alpha * (e0.double() @ W[0].double().t()) + b[0].double() + xa.double()[ia] + xb.double()[ib]).relu()
            h = (h @ W[1].double().t() + b[1].double()).relu()
            ref = torch.nn.functional.layer_norm(h @ W[2].double().t() + b[2].double(), (128,), norm.weight.double(), norm.bias.double(), norm.eps)
        assert torch.isfinite(out).all()
        assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 1e-5, (alpha, scale)


@pytest.mark.parametrize("M", [1, 63, 70_001])
@pytest.mark.parametrize("K", [1, 4, 8, 32])
@pytest.mark.parametrize("relu", [False, True])
def test_linear_narrow128_vs_fp64(M, K, relu):
    """csplat_linear_narrow128 (the encoders' first Linear, K features -> 128; /root/reference/meshnet/graph_network.py:48-111) against the
    fp64 product: plain fp32 FMAs in another order than the library's, 1e-6 of the output scale.  The weight is read with its own
    row stride (a column slice of a wider matrix)."""
    from meshnet.graph_ops import linear_narrow128
    gen = torch.Generator().manual_seed(100 * K + M % 97)
    x = torch.randn(M, K, generator=gen).cuda()
    wide = torch.randn(128, K + 3, generator=gen).cuda()
    W, b = wide[:, 1:K + 1], torch.randn(128, generator=gen).cuda()
    with torch.no_grad():
        out = linear_narrow128(x, W, b, relu=relu)
        ref = x.double() @ W.double().t() + b.double()
        ref = ref.relu() if relu else ref
    assert out.shape == (M, 128) and rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 1e-6


@pytest.mark.parametrize("M,K", [(1, 4), (63, 8), (30_011, 4), (5000, 128)])
def test_mlp3_rows_vs_fp64(M, K):
    """csplat_gnn_mlp3_rows (an encoder's whole MLP + LayerNorm on narrow rows in one launch; /root/reference/meshnet/graph_network.py:48-111)
    against the fp64 composition, inputs of the size of the rollout's edge features (1e-2) and of O(1)."""
    from meshnet.graph_ops import edge_mlp3_pack, mlp3_rows
    for mag in (1e-2, 1.0):
        gen = torch.Generator().manual_seed(M + K)
        x = (torch.randn(M, K, generator=gen) * mag).cuda()
        W0 = (torch.randn(128, K, generator=gen) * (0.5 if K < 128 else 0.1)).cuda()
        W = [(torch.randn(128, 128, generator=gen) * 0.1).cuda() for _ in range(2)]
        b = [torch.randn(128, generator=gen).cuda() * 0.3 for _ in range(3)]
        norm = torch.nn.LayerNorm(128).cuda()
        with torch.no_grad():
            norm.weight.copy_(torch.randn(128, generator=gen)); norm.bias.copy_(torch.randn(128, generator=gen))
            w0 = torch.zeros(128, 128, device="cuda"); w0[:, :K] = W0
            out = mlp3_rows(x, edge_mlp3_pack(w0, W[0], W[1]), b[0], b[1], b[2], norm)
            h = (x.double() @ W0.double().t() + b[0].double()).relu()
            h = (h @ W[0].double().t() + b[1].double()).relu()
            ref = torch.nn.functional.layer_norm(h @ W[1].double().t() + b[2].double(), (128,), norm.weight.double(), norm.bias.double(), norm.eps)
        assert out.shape == (M, 128) and torch.isfinite(out).all()
        assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 1e-5, mag


def test_encoder_rollout_path_vs_module_path():
    """Encoder.forward under no_grad (csplat_linear_narrow128 + csplat_linear128 with ReLU / LayerNorm epilogues, no stock kernel) against the
    same module with autograd on (the training path: library GEMMs + LayerNorm128) and against the fp64 composition."""
    import meshnet.graph_network as gn
    from csplat import native
    torch.manual_seed(4)
    enc = gn.Encoder(8, 128, 4, 128, 2, 128).cuda()
    gen = torch.Generator().manual_seed(5)
    x, e = torch.randn(1201, 8, generator=gen).cuda(), torch.randn(30_011, 4, generator=gen).cuda()
    with torch.no_grad():
        native.prof_enable(["GNN"]); native.prof_read("GNN")
        xn, en = enc(x, e)
        torch.cuda.synchronize()
        _ms, launches = native.prof_read("GNN"); native.prof_enable([])
    assert launches == 2, launches            # one per MLP: csplat_gnn_mlp3_rows (the max |x| pass before it is not a GNN-class launch)
    xg, eg = enc(x, e)
    enc64 = gn.Encoder(8, 128, 4, 128, 2, 128).double().cuda()
    enc64.load_state_dict({k: v.double() for k, v in enc.state_dict().items()})
    with torch.no_grad():
        x64 = enc64.node_fn(x.double()); e64 = enc64.edge_fn(e.double())
    for a, g, r in ((xn, xg, x64), (en, eg, e64)):
        assert rel_err(a.cpu().numpy(), r.cpu().numpy()) < 1e-5
        assert rel_err(a.cpu().numpy(), g.detach().cpu().numpy()) < 1e-5


def test_rollout_with_and_without_the_fused_edge_mlp():
    """EncodeProcessDecode under no_grad with the one-launch edge MLP (graph_network.EDGE_MLP_FUSED = True, the default) and with the
    three launches of rounds 1-4: the same network output to 1e-5, on a graph whose edge count is not a multiple of 64."""
    import meshnet.graph_network as gn
    torch.manual_seed(9)
    net = gn.EncodeProcessDecode(8, 3, 4, 128, 5, 2, 128).cuda()
    gen = torch.Generator().manual_seed(12)
    N, E = 900, 20_011
    ei = torch.randint(0, N, (2, E), generator=gen).cuda()
    x, e = torch.randn(N, 8, generator=gen).cuda(), torch.randn(E, 4, generator=gen).cuda()
    was = gn.EDGE_MLP_FUSED
    try:
        with torch.no_grad():
            gn.EDGE_MLP_FUSED = True
            y1 = net(x, ei, e)
            gn.EDGE_MLP_FUSED = False
            y0 = net(x, ei, e)
    finally:
        gn.EDGE_MLP_FUSED = was
    assert rel_err(y1.cpu().numpy(), y0.cpu().numpy()) < 1e-5


def test_fp16_piece_overflow_is_detected_and_the_call_repeated_with_bf16_pieces():
    """VERDICT r5 item 7 / ADVICE r5: a network whose hidden activations leave fp16's range (a processor edge weight scaled by 1e6) used to
    return NaN rows from the default rollout arithmetic where the reference's fp32 path returns numbers.  EncodeProcessDecode now notices
    (one device word per call), repeats the call with three bf16 pieces and keeps that mode for the module; meshnet.rollout.rollout
    collects the words, reads them once behind its loop and repeats the rollout.  Results against the fp64 oracle of the same network."""
    import warnings
    from meshnet.graph_network import EncodeProcessDecode
    from meshnet.graph_ops import edge_mlp3_mode
    from oracle import gnn_ref
    gen = torch.Generator().manual_seed(21)
    N, E = 500, 6000
    torch.manual_seed(8)
    net = EncodeProcessDecode(8, 3, 4, 128, 2, 2, 128).cuda().eval()
    with torch.no_grad():
        net._processor.gnn_stacks[0].edge_fn[0][0].weight.mul_(1e6)
    x = torch.randn(N, 8, generator=gen).cuda()
    ei = torch.stack([torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)]).cuda()
    ef = torch.randn(E, 4, generator=gen).cuda()
    assert edge_mlp3_mode() == 0
    with torch.no_grad():
        raw = net._forward(x, ei, ef)                                  # the plain fp16-piece path: the overflow is visible
        assert not torch.isfinite(raw).all()
        with warnings.catch_warnings(record=True) as wlist:
            warnings.simplefilter("always")
            out = net(x, ei, ef)
        assert any("bf16" in str(w.message) for w in wlist)
        assert net._bf16_latched and edge_mlp3_mode() == 0             # the library-wide mode is restored, the MODULE keeps bf16
        out2 = net(x, ei, ef)
    p_ = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    ref = gnn_ref.encode_process_decode(p_, x.cpu().numpy(), ei.cpu().numpy(), ef.cpu().numpy())
    assert torch.isfinite(out).all() and rel_err(out.cpu().numpy(), ref) < 1e-4
    assert torch.equal(out, out2)


@pytest.mark.parametrize("real_world", [False, True])
def test_recorded_rollout_equals_the_launch_by_launch_loop(real_world):
    """meshnet.rollout.rollout with its step recorded into a hipGraph (step 0 eager, step 1 recorded, the rest replays) against the same
    loop launched kernel by kernel (graph=False): predictions and final positions BIT-equal -- a replay is the same launches on the same
    buffers.  Latent 128 (the one-launch edge MLP / node update kernels) on a 2,000-node graph, with and without the real_world
    refinement.  Reference loop: train_meshnet_sim.py:126-265."""
    from meshnet import rollout as ro
    from meshnet.cloth_network import ClothMeshSimulator
    dev = "cuda"
    g = torch.Generator().manual_seed(31)
    N, E = 2000, 24_000
    pos = torch.randn(N, 3, generator=g).to(dev)
    ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)]).to(dev)
    torch.manual_seed(4)
    sim = ClothMeshSimulator(3, 8, 4, 128, 3, 2, 128, 2, 2, normalize=False, device=dev).eval()
    hist = (torch.randn(2, N, 3, generator=g) * 0.01).to(dev)
    ntype = torch.randint(0, 2, (N, 1), generator=g).to(dev)
    actions = (torch.randn(7, 3, generator=g) * 0.01).to(dev)
    before = dict(ro.ROLLOUT_STATS)
    a_pred, a_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 7, real_world=real_world, graph=True)
    after = dict(ro.ROLLOUT_STATS)
    assert after["recorded"] == before["recorded"] + 1 and after["replayed_steps"] == before["replayed_steps"] + 6 and \
        after["record_failed"] == before["record_failed"], (before, after)
    b_pred, b_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 7, real_world=real_world, graph=False)
    assert torch.isfinite(a_pred).all()
    assert torch.equal(a_pred, b_pred) and torch.equal(a_pos, b_pos)
    assert torch.equal(a_pred[:, 11], actions)
    # a second rollout of the same combination, from another state: all seven steps are replays of the kept recording
    pos2, hist2 = pos + 0.01, hist * 0.5
    c_pred, c_pos = ro.rollout(sim, pos2, hist2, ntype, ei, actions, 11, 7, real_world=real_world, graph=True)
    again = dict(ro.ROLLOUT_STATS)
    assert again["recorded"] == after["recorded"] and again["replayed_steps"] == after["replayed_steps"] + 7
    d_pred, d_pos = ro.rollout(sim, pos2, hist2, ntype, ei, actions, 11, 7, real_world=real_world, graph=False)
    assert torch.equal(c_pred, d_pred) and torch.equal(c_pos, d_pos)
    # a weight changes: the recording is not replayed (its packed weight images are stale) -- recorded again
    with torch.no_grad():
        sim._encode_process_decode._decoder.node_fn[0].weight.mul_(1.01)
    e_pred, _ = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 7, real_world=real_world, graph=True)
    assert ro.ROLLOUT_STATS["recorded"] == again["recorded"] + 1
    f_pred, _ = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 7, real_world=real_world, graph=False)
    assert torch.equal(e_pred, f_pred) and not torch.equal(e_pred, a_pred)


def _small_rollout_case(seed=51, n_graphs=1, n_actions=6):
    """N = 300, E = 3000, latent 128, 3 message-passing steps: (simulator, positions, history, node types, edge lists, actions)"""
    from meshnet.cloth_network import ClothMeshSimulator
    dev = "cuda"
    g = torch.Generator().manual_seed(seed)
    N, E = 300, 3000
    pos = torch.randn(N, 3, generator=g).to(dev)
    eis = [torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)]).to(dev) for _ in range(n_graphs)]
    torch.manual_seed(seed)
    sim = ClothMeshSimulator(3, 8, 4, 128, 3, 2, 128, 2, 2, normalize=False, device=dev).eval()
    hist = (torch.randn(2, N, 3, generator=g) * 0.01).to(dev)
    ntype = torch.randint(0, 2, (N, 1), generator=g).to(dev)
    actions = (torch.randn(n_actions, 3, generator=g) * 0.01).to(dev)
    return sim, pos, hist, ntype, eis, actions


@pytest.mark.parametrize("real_world", [False, True])
def test_generic_recorded_rollout_equals_the_launch_by_launch_loop(real_world):
    """the GENERIC rollout step (rollout.FUSED_STEP = False: ClothMeshSimulator.predict_velocity and stock tensor operations on state
    buffers) recorded into a hipGraph against the same loop launch by launch: bit-equal predictions and positions; step 0 eager, step 1
    recorded, the rest replays; a second rollout of the combination from another state replays every step of the kept recording; an
    in-place weight change records again.  Reference loop: train_meshnet_sim.py:126-265."""
    from meshnet import rollout as ro
    sim, pos, hist, ntype, (ei,), actions = _small_rollout_case(seed=52, n_actions=5)
    was = ro.FUSED_STEP
    ro.FUSED_STEP = False
    try:
        before = dict(ro.ROLLOUT_STATS)
        a_pred, a_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 5, real_world=real_world, graph=True)
        after = dict(ro.ROLLOUT_STATS)
        assert after["recorded"] == before["recorded"] + 1 and after["replayed_steps"] == before["replayed_steps"] + 4 and \
            after["record_failed"] == before["record_failed"] and after["eager_steps"] == before["eager_steps"] + 1, (before, after)
        b_pred, b_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 5, real_world=real_world, graph=False)
        assert torch.isfinite(a_pred).all()
        assert torch.equal(a_pred, b_pred) and torch.equal(a_pos, b_pos)
        assert torch.equal(a_pred[:, 11], actions)
        pos2, hist2 = pos + 0.01, hist * 0.5
        mid = dict(ro.ROLLOUT_STATS)
        c_pred, c_pos = ro.rollout(sim, pos2, hist2, ntype, ei, actions, 11, 5, real_world=real_world, graph=True)
        again = dict(ro.ROLLOUT_STATS)
        assert again["recorded"] == mid["recorded"] and again["replayed_steps"] == mid["replayed_steps"] + 5 and \
            again["eager_steps"] == mid["eager_steps"], (mid, again)
        d_pred, d_pos = ro.rollout(sim, pos2, hist2, ntype, ei, actions, 11, 5, real_world=real_world, graph=False)
        assert torch.equal(c_pred, d_pred) and torch.equal(c_pos, d_pos) and not torch.equal(c_pred, a_pred)
        # the recording owns its state buffers: what a replayed rollout hands back is a copy, untouched by the next rollout
        c_pos_kept = c_pos.clone()
        ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 5, real_world=real_world, graph=True)
        assert torch.equal(c_pos, c_pos_kept)
        with torch.no_grad():
            sim._encode_process_decode._decoder.node_fn[0].weight.mul_(1.01)
        mid = dict(ro.ROLLOUT_STATS)
        e_pred, _ = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 5, real_world=real_world, graph=True)
        assert ro.ROLLOUT_STATS["recorded"] == mid["recorded"] + 1
        f_pred, _ = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 5, real_world=real_world, graph=False)
        assert torch.equal(e_pred, f_pred) and not torch.equal(e_pred, a_pred)
    finally:
        ro.FUSED_STEP = was


def test_a_recording_is_kept_across_rollouts_of_another_length():
    """the fused step's recording is keyed on the capacity of its action / prediction buffers (64 rows at least), not on nsteps: a
    6-step rollout records, a 5-step rollout of the same combination replays every step; both bit-equal to the eager loop"""
    from meshnet import rollout as ro
    sim, pos, hist, ntype, (ei,), actions = _small_rollout_case(seed=53)
    assert ro.FUSED_STEP and ro._FusedClothStep.applicable(sim, pos, hist, ntype, ei, actions, 11)
    before = dict(ro.ROLLOUT_STATS)
    a_pred, a_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 6, graph=True)
    after = dict(ro.ROLLOUT_STATS)
    assert after["recorded"] == before["recorded"] + 1 and after["replayed_steps"] == before["replayed_steps"] + 5, (before, after)
    b_pred, b_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 5, graph=True)
    again = dict(ro.ROLLOUT_STATS)
    assert again["recorded"] == after["recorded"] and again["replayed_steps"] == after["replayed_steps"] + 5 and \
        again["eager_steps"] == after["eager_steps"], (after, again)
    c_pred, c_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 6, graph=False)
    d_pred, d_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 5, graph=False)
    assert torch.isfinite(a_pred).all() and a_pred.shape[0] == 6 and b_pred.shape[0] == 5
    assert torch.equal(a_pred, c_pred) and torch.equal(a_pos, c_pos)
    assert torch.equal(b_pred, d_pred) and torch.equal(b_pos, d_pos)


def test_rollout_recordings_are_evicted_first_in_first_out_at_two():
    """three graphs in turn: never more than _ROLLOUT_CACHE_MAX = 2 recordings are kept, and the first combination -- evicted by the
    third -- records again when it returns"""
    from meshnet import rollout as ro
    sim, pos, hist, ntype, eis, actions = _small_rollout_case(seed=54, n_graphs=3)
    assert ro._ROLLOUT_CACHE_MAX == 2
    preds = []
    for ei in eis:
        before = ro.ROLLOUT_STATS["recorded"]
        preds.append(ro.rollout(sim, pos, hist, ntype, ei, actions, 11, 5, graph=True)[0])
        assert ro.ROLLOUT_STATS["recorded"] == before + 1 and len(ro._ROLLOUT_CACHE) <= 2
    before = dict(ro.ROLLOUT_STATS)
    ro.rollout(sim, pos, hist, ntype, eis[2], actions, 11, 5, graph=True)             # the newest is still there: replays only
    assert ro.ROLLOUT_STATS["recorded"] == before["recorded"] and ro.ROLLOUT_STATS["replayed_steps"] == before["replayed_steps"] + 5
    again, _ = ro.rollout(sim, pos, hist, ntype, eis[0], actions, 11, 5, graph=True)
    assert ro.ROLLOUT_STATS["recorded"] == before["recorded"] + 1 and len(ro._ROLLOUT_CACHE) <= 2
    assert torch.equal(again, preds[0])


def test_rollout_repeats_with_bf16_pieces_after_an_overflow():
    """a rollout whose network leaves fp16's range at some step: the per-call overflow words are collected without a host read, read once
    behind the loop, and the rollout is repeated from its start with three bf16 pieces -- finite results equal to the launch-by-launch
    loop under csplat_gnn_edge_mlp3_mode(1)."""
    import warnings
    from meshnet import rollout as ro
    from meshnet.cloth_network import ClothMeshSimulator
    from meshnet.graph_ops import edge_mlp3_mode
    dev = "cuda"
    g = torch.Generator().manual_seed(33)
    N, E = 1500, 18_000
    pos = torch.randn(N, 3, generator=g).to(dev)
    ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)]).to(dev)
    hist = (torch.randn(2, N, 3, generator=g) * 0.01).to(dev)
    ntype = torch.randint(0, 2, (N, 1), generator=g).to(dev)
    actions = (torch.randn(5, 3, generator=g) * 0.01).to(dev)

    def build():
        torch.manual_seed(6)
        sim = ClothMeshSimulator(3, 8, 4, 128, 2, 2, 128, 2, 2, normalize=False, device=dev).eval()
        with torch.no_grad():
            sim._encode_process_decode._processor.gnn_stacks[1].edge_fn[0][0].weight.mul_(1e6)
            sim._encode_process_decode._decoder.node_fn[-2].weight.mul_(1e-3)      # (keep the velocities small: the state must stay finite)
        return sim
    sim = build()
    before = dict(ro.ROLLOUT_STATS)
    with warnings.catch_warnings(record=True):
        warnings.simplefilter("always")
        pred, pos_end = ro.rollout(sim, pos, hist, ntype, ei, actions, 3, 5)
    assert ro.ROLLOUT_STATS["repeated_bf16"] == before["repeated_bf16"] + 1
    assert torch.isfinite(pred).all() and torch.isfinite(pos_end).all() and sim._encode_process_decode._bf16_latched
    ref_sim = build()
    was = edge_mlp3_mode(1)
    try:
        ref_pred, ref_pos = ro.rollout(ref_sim, pos, hist, ntype, ei, actions, 3, 5, graph=False)
    finally:
        edge_mlp3_mode(was)
    assert torch.equal(pred, ref_pred) and torch.equal(pos_end, ref_pos)


@pytest.mark.parametrize("normalize", [False, True])
def test_fused_rollout_step_equals_the_module_path(normalize):
    """meshnet.rollout._FusedClothStep (round 6: the rollout step as library launches only -- head, ordered edge features, encoders,
    processor, decoder layers, decode, integrate; the step number on the device) against the generic step that calls
    ClothMeshSimulator.predict_velocity and stock tensor operations (CSPLAT_ROLLOUT_FUSED=0's path), with and without trained-like
    normaliser statistics: predictions and final positions to 1e-5 of their scale (the decoder's last Linear and the 128-wide layers sum
    in another order than the library GEMMs), the grasped node pinned exactly.  Reference: cloth_network.py:72-193,
    train_meshnet_sim.py:126-265."""
    from meshnet import rollout as ro
    from meshnet.cloth_network import ClothMeshSimulator
    dev = "cuda"
    g = torch.Generator().manual_seed(41)
    N, E = 1200, 15_000
    pos = torch.randn(N, 3, generator=g).to(dev)
    ei = torch.stack([torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)]).to(dev)
    torch.manual_seed(9)
    sim = ClothMeshSimulator(3, 8, 4, 128, 3, 2, 128, 2, 2, normalize=normalize, device=dev)
    if normalize:            # statistics as a few training batches would leave them
        sim.train()
        with torch.no_grad():
            for _ in range(3):
                sim._node_normalizer(torch.randn(N, 8, generator=g).to(dev) * 0.3 + 0.1, True)
                sim._output_normalizer(torch.randn(N, 3, generator=g).to(dev) * 0.02, True)
    sim.eval()
    hist = (torch.randn(2, N, 3, generator=g) * 0.01).to(dev)
    ntype = torch.randint(0, 2, (N, 1), generator=g).to(dev)
    actions = (torch.randn(6, 3, generator=g) * 0.01).to(dev)
    assert ro._FusedClothStep.applicable(sim, pos, hist, ntype, ei, actions, 5)
    a_pred, a_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, 5, 6)
    was = ro.FUSED_STEP
    ro.FUSED_STEP = False
    try:
        b_pred, b_pos = ro.rollout(sim, pos, hist, ntype, ei, actions, 5, 6, graph=False)
    finally:
        ro.FUSED_STEP = was
    assert torch.isfinite(a_pred).all()
    assert rel_err(a_pred.cpu().numpy(), b_pred.cpu().numpy()) < 1e-5 and rel_err(a_pos.cpu().numpy(), b_pos.cpu().numpy()) < 1e-5
    assert torch.equal(a_pred[:, 5], actions)


@pytest.mark.parametrize("em_mode", [0, 1])
@pytest.mark.parametrize("N", [1, 31, 1000, 10_007])
def test_rows_chain_matches_fp64(N, em_mode):
    """csplat_gnn_rows_chain (round 6: the first processor layer's x_i / x_j products and the decoder's two hidden layers on pre-packed
    16-bit pieces, one launch each): both modes against the fp64 composition, 1e-5 of each output's scale, node latents of O(1) and of
    O(100); rows past a multiple of 32; both arithmetic modes (two fp16 pieces / three bf16 pieces).  Reference: graph_network.py:178-199,
    :295-332."""
    from meshnet.graph_ops import edge_mlp3_mode, rows_chain, rows_chain_pack
    gen = torch.Generator().manual_seed(100 + N)
    was = edge_mlp3_mode(em_mode)
    try:
        for scale in (1.0, 100.0):
            x = (torch.randn(N, 128, generator=gen) * scale).cuda()
            W = [(torch.randn(128, 128, generator=gen) * 0.1).cuda() for _ in range(2)]
            b = [(torch.randn(128, generator=gen) * 0.3).cuda() for _ in range(2)]
            with torch.no_grad():
                a, c = rows_chain(x, rows_chain_pack(0, W[0], W[1]), 0)
                h = rows_chain(x, rows_chain_pack(1, W[0], W[1]), 1, b[0], b[1])
            xd = x.double()
            ra, rc = xd @ W[0].double().t(), xd @ W[1].double().t()
            rh = ((xd @ W[0].double().t() + b[0].double()).relu() @ W[1].double().t() + b[1].double()).relu()
            for got, ref in ((a, ra), (c, rc), (h, rh)):
                assert got.shape == ref.shape and rel_err(got.cpu().numpy(), ref.cpu().numpy()) < 1e-5
    finally:
        edge_mlp3_mode(was)
