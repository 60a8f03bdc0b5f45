"""The head of the train step: the cloth regularisers of train_utils.py:76-237 (deformation magnitude, rigid edge length, momentum) as one
launch (FusedClothRegs), fused with the time-conditioned simulator into one autograd node (SimulatorStep), and the queue that lets the
step issue that launch behind the rasterizer's forward (launch_deferred).  Re-exported by csplat.train."""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import native as _n
from .image_loss import _IMG_SCRATCH


def _cloth_regs_for(ctx, D, edge_index, rest_len, lams, csr, defer):
    """csplat_cloth_regs on the vertices D [T,V,3] for an autograd node -> (loss, grad).  The kernel writes into `loss` / `grad`, which
    exist already: WHEN it is launched is the caller's choice -- now, or with defer queued for launch_deferred() (e.g. behind the
    rasterizer's forward, off the step's critical path); ctx.pending keeps the queue entry for the node's backward."""
    T, V, E = int(D.shape[0]), int(D.shape[1]), int(edge_index.shape[1])
    loss = torch.empty((), dtype=torch.float32, device=D.device)
    grad = torch.empty_like(D)
    ei, rl = edge_index.contiguous(), rest_len.contiguous().float()
    dev, stream, skey = D.device, _n.stream_handle(D.device), _n.scratch_stream(D.device)

    def launch():
        with _n.on_device(dev):
            # zeroed once per (device, stream, sizes): the kernel leaves its ticket at zero
            scratch = _IMG_SCRATCH.buffer(dev, ("regs", T, V, E), lambda: _n.lib.csplat_cloth_regs_scratch_bytes(T, V, E), stream=skey)
            _n.check(_n.lib.csplat_cloth_regs(stream, T, V, E, _n.ptr(D), _n.ptr(ei), _n.ptr(rl), *[float(v) for v in lams], _n.ptr(loss),
                                              _n.ptr(grad), _n.ptr(scratch), *([None] * 4 if csr is None else [_n.ptr(c) for c in csr])),
                     "csplat_cloth_regs")
    if defer:
        ctx.pending = _defer(launch)
    else:
        ctx.pending = None
        launch()
    return loss, grad


class FusedClothRegs(torch.autograd.Function):
    """the three cloth regularisers and their gradient in one launch (csplat_cloth_regs); backward scales the stored gradient."""

    @staticmethod
    def forward(ctx, D, edge_index, rest_len, lam_deform, lam_rigid, lam_mom, csr=None, tap=False, defer=False):
        D = D.contiguous().float()
        ctx.set_materialize_grads(False)
        loss, grad = _cloth_regs_for(ctx, D, edge_index, rest_len, (lam_deform, lam_rigid, lam_mom), csr, defer)
        ctx.save_for_backward(grad)
        ctx.tap = bool(tap)
        if tap:     # D passes through: the gradient arriving for it and the regularisers' own leave as ONE tensor (one launch)
            return loss, D.view_as(D)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g, g_through=None):
        _issue(ctx.pending)
        (grad,) = ctx.saved_tensors
        if ctx.tap and g_through is not None:
            out = torch.addcmul(g_through, grad, g) if g is not None else g_through
        else:
            out = grad * g if g is not None else None
        return out, None, None, None, None, None, None, None, None


class SimulatorStep(torch.autograd.Function):
    """The head of a training step as ONE autograd node: the time-conditioned simulator for the step's T cameras
    (meshnet_network.py:361-373 per time: hidden layers, output layer, + the table rows) AND the cloth regularisers of its output
    (train_utils.py:83-102) -- graph_ops.SimResidual followed by FusedClothRegs(tap=True): the same three forward launches (the
    regularisers' queued for launch_deferred()) and three backward launches, two nodes less to record and to walk.
    Returns (vertices [T,V,3], regulariser loss)."""

    @staticmethod
    def forward(ctx, e, W1, b1, W2, b2, Wo, bo, base, edge_index, rest_len, lam_deform, lam_rigid, lam_mom, csr, defer=False):
        from meshnet import graph_ops as go
        ctx.sinks = tuple(_n.grad_sink(t) for t in (W1, b1, W2, b2, Wo, bo))       # (csplat.dist.FlatGrads: gradients written in place)
        e, W2s, h1, h2 = go._sim_hidden_fwd(e, W1, b1, W2, b2)
        y, h2, Wo = go._rows_dot_fwd(h2, Wo, bo, base)
        D = y.view(int(e.shape[0]), -1, 3)
        loss, grad = _cloth_regs_for(ctx, D, edge_index, rest_len, (lam_deform, lam_rigid, lam_mom), csr, defer)
        ctx.save_for_backward(e, W2s, h1, h2, Wo, grad)
        ctx.set_materialize_grads(False)
        return D, loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_D, g_loss):
        from meshnet import graph_ops as go
        _issue(ctx.pending)
        e, W2s, h1, h2, Wo, grad = ctx.saved_tensors
        if g_D is None and g_loss is None:
            return (None,) * 15
        if g_D is None:
            g = grad * g_loss
        else:
            g = g_D.contiguous().float() if g_loss is None else torch.addcmul(g_D, grad, g_loss)
        dWo, dbo, dh = go._rows_dot_bwd(Wo, h2, g, sinks=ctx.sinks[4:6])
        dW1, db1, dW2, db2 = go._sim_hidden_bwd(e, W2s, h1, h2, dh, sinks=ctx.sinks[:4])
        return (None, dW1, db1, dW2, db2, dWo, dbo) + (None,) * 8


def simulator_step(simulator, times, gaussians, opt, defer=False, static=None):
    """(vertices [T,V,3], regulariser loss) through SimulatorStep when the simulator is the time-conditioned residual MLP on the GPU and
    the fused regularisers apply; None otherwise (the caller composes forward_times + regularization).  defer=True: the regularisers'
    kernel is queued, the caller MUST run launch_deferred() before the loss is consumed.  static = (code [T,K0], table rows [T,V,3]):
    the parameter-free inputs of the camera times in buffers of the caller's (CapturedStep refills them between replays)."""
    from meshnet import graph_ops as go
    need = ("times_on_device", "input", "hidden", "output")
    if not all(hasattr(simulator, a) for a in need) or len(times) > 8 or len(times) == 0:
        return None
    if static is not None:
        enc, base = static
    else:
        _tt, enc, base = simulator.times_on_device(times)
    if not go.sim_residual_applies(enc, simulator.input, simulator.hidden, simulator.output, base):
        return None
    csr = _cloth_edge_csr(gaussians, int(base.shape[1]))
    s = simulator
    return SimulatorStep.apply(enc, s.input.weight, s.input.bias, s.hidden.weight, s.hidden.bias, s.output.weight, s.output.bias, base,
                               gaussians.mesh.edge_index, gaussians.edge_norm.reshape(-1), *_cloth_lambdas(opt), csr, bool(defer))


_DEFERRED = []


def _defer(launch):
    """queue a launch for launch_deferred(); returns the queue entry [launch, issued] the node keeps: its backward issues a launch that
    nobody issued (regularization(..., defer=True) outside train_step -- ADVICE r3: the gradient would be read uninitialised; the LOSS
    value is only defined once the launch has been issued, which is the caller's contract with defer=True)"""
    ent = [launch, False]
    _DEFERRED.append(ent)
    return ent


def _issue(ent):
    if ent is None:
        return
    # the entry leaves the queue BEFORE its launch runs: a launch that raises must not stay at the head (launch_deferred would spin on an
    # entry already marked issued -- ADVICE r4)
    _DEFERRED[:] = [e for e in _DEFERRED if e is not ent]
    if not ent[1]:
        ent[1] = True
        fn, ent[0] = ent[0], None       # (the closure holds the node's tensors: drop it with the launch -- kept on the ctx it is a
        fn()                            #  reference cycle through the node's own output, and memory of a graph's private pool then
        #                                  outlives the capture: a segfault at capture_end, measured)


def launch_deferred():
    """launches what FusedClothRegs(defer=True) queued (same stream, in order); a no-op otherwise"""
    while _DEFERRED:
        _issue(_DEFERRED.pop(0))


def edge_csr(edge_index, n_nodes):
    """(dst_rowptr, dst_perm, src_rowptr, src_perm), int32: edge ids grouped by target / source vertex, ascending in a group."""
    out = []
    for row in (1, 0):
        out += list(_n.group_by_key(edge_index[row], n_nodes))
    return tuple(out)


def _cloth_lambdas(opt):
    """(lambda_deform_mag, lambda_rigid, lambda_momentum) as the fused kernel takes them: a weight that is not > 0 is 0"""
    return (opt.lambda_deform_mag if opt.lambda_deform_mag > 0. else 0., opt.lambda_rigid if opt.lambda_rigid > 0 else 0.,
            opt.lambda_momentum if opt.lambda_momentum > 0 else 0.)


def _cloth_edge_csr(gaussians, n_vertices):
    """edge_csr of the Gaussians' cloth graph, cached on the object (the graph is static: its CSR is built once); an object that
    refuses the attribute gets a fresh one every call"""
    ei = gaussians.mesh.edge_index
    key = (ei.data_ptr(), ei._version, tuple(ei.shape), n_vertices)
    cache = getattr(gaussians, "_edge_csr", None)
    if cache is None or cache[0] != key:
        cache = (key, edge_csr(ei, n_vertices))
        try:
            gaussians._edge_csr = cache
        except Exception:
            pass
    return cache[1]


def regularization(all_vertice_deform, gaussians, opt, static=False, fused=True, tap=False, defer=False):
    """train_utils.py:76-237 (the active terms).  On the GPU the terms and their gradient come from one kernel
    (FusedClothRegs); fused=False composes them from torch ops as upstream does (the parity reference of the tests).
    tap=True returns (loss, vertices): `vertices` is all_vertice_deform passed THROUGH the regulariser node -- render from it and the
    two gradients of the vertices (image path, regularisers) are combined in the node's backward instead of by autograd (one launch
    instead of a multiply and an add).  defer=True (with tap, on the fused path): the kernel is queued, not launched -- the caller runs
    launch_deferred() once the work that must not wait for it (the rasterizer's forward) has been issued."""
    n_cams = all_vertice_deform.shape[0]
    if fused and not static and all_vertice_deform.is_cuda and all_vertice_deform.dim() == 3:
        lams = _cloth_lambdas(opt)
        ei, csr = gaussians.mesh.edge_index, _cloth_edge_csr(gaussians, int(all_vertice_deform.shape[1]))
        if tap and all_vertice_deform.dtype == torch.float32 and all_vertice_deform.is_contiguous():
            return FusedClothRegs.apply(all_vertice_deform, ei, gaussians.edge_norm.reshape(-1), *lams, csr, True, bool(defer))
        loss = FusedClothRegs.apply(all_vertice_deform, ei, gaussians.edge_norm.reshape(-1), *lams, csr)
        return (loss, all_vertice_deform) if tap else loss
    if tap:
        return regularization(all_vertice_deform, gaussians, opt, static, fused), all_vertice_deform
    if fused and not static:
        _n.composed_fallback("train.regularization", "shape", all_vertice_deform)
    loss = torch.zeros([], device=all_vertice_deform.device)
    if not static and opt.lambda_deform_mag > 0. and n_cams >= 3:
        d0 = torch.linalg.norm(all_vertice_deform[1] - all_vertice_deform[0], dim=-1).mean()
        d1 = torch.linalg.norm(all_vertice_deform[2] - all_vertice_deform[1], dim=-1).mean()
        loss = loss + opt.lambda_deform_mag * 0.5 * (d0 + d1)
    if not static and opt.lambda_rigid > 0:
        ei = gaussians.mesh.edge_index
        # (index_select: its backward is an atomic index_add; advanced indexing would sort the 2E indices every step)
        disp = all_vertice_deform.index_select(1, ei[1]) - all_vertice_deform.index_select(1, ei[0])
        deformed_norm = torch.linalg.norm(disp, dim=-1, keepdim=True)
        static_norm = gaussians.edge_norm.unsqueeze(0).expand(n_cams, -1, -1)
        loss = loss + opt.lambda_rigid * F.l1_loss(static_norm, deformed_norm)
    if not static and opt.lambda_momentum > 0 and n_cams >= 3:
        m = all_vertice_deform[2] - 2 * all_vertice_deform[1] + all_vertice_deform[0]
        loss = loss + opt.lambda_momentum * torch.linalg.norm(m, dim=-1, ord=1).mean()
    return loss
