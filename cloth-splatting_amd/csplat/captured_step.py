"""train_step recorded into a hipGraph and replayed (CapturedStep): what train_step(captured=True) runs.  It calls csplat.train.train_step
with the `_cap` record both to record a step and, eagerly, for whatever a recording does not cover.  Re-exported by csplat.train."""
from types import SimpleNamespace

import ctypes as C

import torch

from . import native as _n
from .graphs import capture, caps_from_counts


class CapturedStep:
    """train_step recorded ONCE into a hipGraph and replayed (the reference times its step with an event pair around
    the loop body, train.py:146,178 -- the GPU work of a step, which is what a replayed graph costs).

    The eager step is bound by the host: ~33 launches of 5-300 us, ~25 us of Python and launch overhead each, and one read of the
    forward's counts in the middle.  Recorded, the launches cost the host nothing -- which needs a step without a single per-step host
    value in its launches:
      * the rasterizer's forward is launched ON FAITH (csplat_forward_views_faith): both phases with capacities from the last eager
        step's counts + 1/8, nothing read back; a device word `valid` says whether the counts fitted, every kernel of the second phase
        and of the backward leaves an unfitting step alone, and BOTH Adam steps honour the same word (csplat_adam_step_dev: step count
        and learning rates on the device too) -- a miss changes no parameter, no moment, no count;
      * camera matrices, the simulator's time inputs and the ground-truth images live in buffers of this object that are refilled
        between replays (only when the cameras changed);
      * ONE host read per step, at its end: [valid, PSNR, loss, the views' counts] arrive in pinned memory through a copy node of the
        graph.  valid == 0 -> the step is repeated eagerly (exact sizes) and the graph is re-recorded with new capacities at the next
        call; counts within 3 % of a capacity re-record too, before a miss happens.
    One graph per step SHAPE: (number of cameras, image size, field of view, number of Gaussians, active SH degree, parameter storage,
    pipe.antialiasing).
    Falls back to the eager train_step for what it does not cover: masks, a static stage, view-parallel runs, densification steps and
    every optional term that is on (train._optional_terms_on: opt.lambda_depth / opt.lambda_silhouette, opt.lambda_chamfer,
    opt.lambda_isometric / opt.lambda_spring / opt.lambda_rigidity, opt.lambda_flow > 0) -- the rasterizer refuses the geometry terms'
    gradients on a forward launched on faith, the observed clouds' sizes are per camera and not part of a step's shape, the kNN graph
    is refreshed on the host's schedule, and the flow images belong to the cameras of a step, not to its shape."""

    def __init__(self, gaussians, simulator, meshnet_optimizer, pipe=None, opt=None, background=None):
        from . import train as tr       # (at call time: csplat.train imports this module)
        pipe, opt = tr.DEFAULT_PIPE if pipe is None else pipe, tr.DEFAULT_OPT if opt is None else opt
        self.g, self.sim, self.mopt, self.pipe, self.opt, self.bg = gaussians, simulator, meshnet_optimizer, pipe, opt, background
        self.graphs = {}
        self.stats = {"eager": 0, "recorded": 0, "replayed": 0, "missed": 0, "rerecorded_early": 0}

    def matches(self, simulator, meshnet_optimizer, pipe, opt, background):
        return simulator is self.sim and meshnet_optimizer is self.mopt and pipe is self.pipe and opt is self.opt and background is self.bg

    # ---- shape of a step
    def _key(self, cams):
        c0 = cams[0]
        g = self.g
        return (len(cams), int(c0.image_height), int(c0.image_width), float(c0.FoVx), float(c0.FoVy), int(g.num_gaussians),
                int(g.active_sh_degree), tuple(int(p.data_ptr()) for p in g.parameters()),
                tuple(int(p.data_ptr()) for p in self.sim.parameters()), bool(getattr(self.pipe, "antialiasing", False)))

    def _coverable(self, cams):
        from .optim import GroupedAdam
        from .train import _optional_terms_on
        return (len(cams) >= 2 and len(cams) <= 8 and all(getattr(c, "mask", None) is None for c in cams) and
                not _optional_terms_on(self.opt) and
                len({(int(c.image_height), int(c.image_width), float(c.FoVx), float(c.FoVy)) for c in cams}) == 1 and
                self.g.mesh.pos.is_cuda and isinstance(self.g.optimizer, GroupedAdam) and isinstance(self.mopt, GroupedAdam) and
                not (int(_n.lib.csplat_debug_flags_query()) & _n.DEBUG_UNBATCHED) and      # (global sort, per-view launches; the bit-reproducible K7, bit 8, is served by the batched path since round 6)
                all(hasattr(self.sim, a) for a in ("times_on_device", "input", "hidden", "output")))

    def _eager(self, iteration, cams, key=None):
        """the step as an ordinary train_step; with `key`, its counts become the capacities the shape's next call records with"""
        import diff_gaussian_rasterization as dgr
        from .train import train_step
        self.stats["eager"] += 1
        with dgr.forward_mode(keep_info=True):      # (the step's counts stay readable on the device: the next recording's capacities)
            out = train_step(iteration, cams, self.g, self.sim, self.mopt, self.pipe, self.opt, self.bg)
        if key is not None and dgr.LAST_INFO:
            if len(self.graphs) >= 8:
                self.graphs.clear()
            self._pend(key, caps_from_counts(torch.stack(list(dgr.LAST_INFO)).cpu().tolist()))
        return out

    def _pend(self, key, caps):
        """the shape `key` is recorded at its next call, with the capacities `caps`"""
        st = self.graphs[key] = {"graph": None, "pending_caps": caps}
        return st

    # ---- static inputs
    def _fill(self, st, cams):
        """the cameras of this call -> the graph's input buffers (skipped when they are the objects of the previous call)"""
        if st["cams_seen"] is not None and len(st["cams_seen"]) == len(cams) and all(a is b for a, b in zip(st["cams_seen"], cams)) and \
                st["times_seen"] == tuple(float(c.time) for c in cams):
            return
        dev = st["gt"].device
        for i, c in enumerate(cams):
            st["view"][i].copy_(c.world_view_transform.to(dev).reshape(16), non_blocking=True)
            st["proj"][i].copy_(c.full_proj_transform.to(dev).reshape(16), non_blocking=True)
            st["campos"][i].copy_(c.camera_center.to(dev).reshape(3), non_blocking=True)
            st["gt"][i].copy_(c.original_image.to(dev), non_blocking=True)
        _tt, enc, base = self.sim.times_on_device([c.time for c in cams])
        st["enc"].copy_(enc)
        st["base"].copy_(base.reshape(st["base"].shape))
        st["cams_seen"], st["times_seen"] = list(cams), tuple(float(c.time) for c in cams)

    def _record(self, key, cams, caps):
        import diff_gaussian_rasterization as dgr
        from .train import train_step
        g = self.g
        dev = g.face_bary.device
        T = len(cams)
        c0 = cams[0]
        H, W = int(c0.image_height), int(c0.image_width)
        _tt, enc, base = self.sim.times_on_device([c.time for c in cams])
        st = {"view": torch.zeros(T, 16, device=dev), "proj": torch.zeros(T, 16, device=dev), "campos": torch.zeros(T, 3, device=dev),
              "gt": torch.zeros(T, 3, H, W, device=dev), "enc": torch.zeros_like(enc), "base": torch.zeros_like(base),
              "valid": torch.zeros(1, dtype=torch.int32, device=dev), "cams_seen": None, "times_seen": None, "caps": tuple(int(c) for c in caps)}
        scams = [SimpleNamespace(image_height=H, image_width=W, FoVx=c0.FoVx, FoVy=c0.FoVy, world_view_transform=st["view"][i].view(4, 4),
                                 full_proj_transform=st["proj"][i].view(4, 4), camera_center=st["campos"][i], time=float(cams[i].time),
                                 original_image=st["gt"][i], mask=None) for i in range(T)]
        self._fill(st, cams)
        g.optimizer.captured_setup()
        self.mopt.captured_setup()
        for p in list(g.parameters()) + list(self.sim.parameters()):
            p.grad = None
        torch.cuda.synchronize(dev)
        graph = torch.cuda.CUDAGraph()
        faith = {"caps": st["caps"], "valid": st["valid"]}
        n_log = 4 + 3 * T
        st["host"] = torch.zeros(n_log, dtype=torch.float32).pin_memory()
        st["host_seq"] = torch.full((1,), -1.0, dtype=torch.float32).pin_memory()
        st["packed"] = torch.zeros(n_log, dtype=torch.float32, device=dev)
        seq_src = g.optimizer._cap["state"]        # steps taken BEFORE this one: the host knows the value it waits for

        def log(psnr_t, loss_t):
            srcs = [seq_src, st["valid"], psnr_t.reshape(1), loss_t.reshape(1)] + list(faith["info"])
            kinds = [1, 1, 0, 0] + [2] * T          # (the views' counts travel as raw int32 bits: exact at any size)
            counts = [1, 1, 1, 1] + [3] * T
            n = len(srcs)
            keep = [t if t.dtype in (torch.float32, torch.int32) else t.float() for t in srcs]
            _n.launch("csplat_gather_words", dev, n, _n.ptr_table(keep), (C.c_int * n)(*kinds), (C.c_int * n)(*counts), _n.ptr(st["packed"]))
            # two copy nodes: the line, then the word the host spins on -- when the second has landed the first has
            st["host"].copy_(st["packed"], non_blocking=True)
            st["host_seq"].copy_(st["packed"][0:1], non_blocking=True)
            st["_keep"] = keep
        with dgr.forward_mode(faith=faith, replay_device=dev):
            with capture(graph):          # (the cyclic collector is held off during the capture: csplat/graphs.py)
                ps, loss, stats = train_step(0, scams, g, self.sim, self.mopt, self.pipe, self.opt, self.bg,
                                             _cap={"sim_in": (st["enc"], st["base"]), "gt": st["gt"], "valid": st["valid"], "log": log})
        # what the recording's raw pointers depend on: the ticketed scratch caches and both optimizers' device words
        st.update(graph=graph, psnr=ps, loss=loss, stats=stats, epochs=self._epochs())
        self.graphs[key] = st
        self.stats["recorded"] += 1
        return st

    def _epochs(self):
        return (_n.SCRATCH_EPOCH[0], self.g.optimizer.__dict__.get("_cap", {}).get("epoch"), self.mopt.__dict__.get("_cap", {}).get("epoch"))

    def __call__(self, iteration, cams):
        cams = list(cams)
        # (a step that raises the SH degree, and whatever the graph does not cover, is an ordinary train_step)
        if iteration % 1000 == 0 or not self._coverable(cams):
            return self._eager(iteration, cams)
        key = self._key(cams)
        st = self.graphs.get(key)
        if st is None:
            # first step of a shape: eager -- it creates the optimizer state and leaves the exact counts the capacities are taken from
            return self._eager(iteration, cams, key)
        if st.get("graph") is not None and st["epochs"] != self._epochs():
            # a scratch cache was evicted (an entry point failed, a cache overflowed) or an optimizer's device words were re-allocated since
            # this graph was recorded: its raw pointers may be dangling -- never replay it; record again with the same capacities
            self.stats["rerecorded_stale"] = self.stats.get("rerecorded_stale", 0) + 1
            st = self._pend(key, st["caps"])
        if st.get("graph") is None:
            st = self._record(key, cams, st["pending_caps"])
        else:
            self._fill(st, cams)
        self.g.optimizer.captured_refresh_lr()
        self.mopt.captured_refresh_lr()
        expect = float(int(self.g.optimizer._cap["items"][0][1]["step"].item()))      # (a CPU tensor: the host-side step counter)
        st["host_seq"][0] = -1.0            # (the previous replay's copies have landed: its line was read)
        st["graph"].replay()
        # the step's log line leaves the GPU right behind the image loss -- half a step before the step ends -- and the host only waits for
        # THAT: it returns to the caller (and issues the next replay) while the backward and the optimizer steps still run
        host, seq = st["host"], st["host_seq"]
        spins = 0
        while float(seq[0]) != expect:
            spins += 1
            if spins > 200000:          # (seconds: something is wrong -- fall back to the stream)
                torch.cuda.current_stream(st["gt"].device).synchronize()
                if float(seq[0]) != expect:
                    raise RuntimeError(f"CapturedStep: the recorded step reported step count {float(seq[0])}, expected {expect}")
                break
        if float(host[1]) != 1.0:           # the counts outgrew the capacities: nothing was applied -- repeat eagerly, re-record next time
            self.stats["missed"] += 1
            self.graphs.pop(key, None)
            return self._eager(iteration, cams, key)
        self.stats["replayed"] += 1
        self.g.optimizer.captured_advance_host()
        self.mopt.captured_advance_host()
        T = len(cams)
        counts = host[4:4 + 3 * T].view(torch.int32).view(T, 3)
        caps = st["caps"]
        psnr_v, loss_v = host[2].clone(), host[3].clone()        # (the pinned line is overwritten by the next replay)
        if int(counts[:, 0].max()) > 0.97 * caps[0] or int(counts[:, 1].max()) > 0.97 * caps[1] or int(counts[:, 2].max()) > 0.97 * caps[2]:
            # close to a capacity: re-record with room before a step is lost (the results of this replay are final -- copies are returned)
            self._pend(key, caps_from_counts(counts.tolist()))
            self.stats["rerecorded_early"] += 1
            return psnr_v, loss_v, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st["stats"].items()}
        return psnr_v, loss_v, dict(st["stats"])
