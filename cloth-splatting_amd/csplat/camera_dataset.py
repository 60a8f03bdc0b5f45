"""The camera data set of the reconstruction side: the reference's MDNerfDataset (scene_reconstruction/dataset.py:46-123), a view x time grid
of cameras with `get_one_item` and a three-consecutive-timesteps `__getitem__`, with its images RESIDENT ON THE DEVICE.

The reference keeps float images on the host and builds a fresh Camera per item, so every training step begins with host-to-device copies
(or, for a caller who keeps them on the device, a torch.cat) of three ground-truth images and three masks.  Here

  * the images and masks live in one device buffer of slots that grows geometrically (`add_frames` uploads only the (view, time) cells that
    are not there yet: the online loop re-reads a growing scene every round).  The loader's images are 8-bit levels divided by 255
    (scene_io.py), so by default they are stored as those levels -- a quarter of the float32 size, nothing lost -- and as float32 words when
    some image or mask is not such a quotient (`storage`);
  * `step(view, time_ids)` produces the step's `gt [n,3,H,W]` and `mask [n,1,H,W]` in ONE launch (csplat_camera_batch,
    csrc/csplat_camera_dataset.hip) from slot indices that travel through one small pinned upload -- through none when that set of
    slots was uploaded before, or after `plan(schedule)` has uploaded the indices of a whole schedule -- and returns a CameraBatch: a
    list of cameras with the fields of scene_io.camera_from_info, bit for bit.  Their matrix tensors are views of persistent per-slot device tables (stable identities
    across steps), `original_image = gt[i]`, `mask = mask[i]`, and each camera carries `gt_stack`, `gt_index` and `mask_stack`, which
    csplat.train's `_gt_stack` and mask concatenation hand through instead of concatenating.

The grid rules are the reference's: `viewpoint_ids` / `time_ids` are the sorted unique ids and a grid position is the POSITION of an id in
them (:54-71); `__getitem__(view)` is three consecutive times around a middle one uniform in [1, n_times - 2] when n_times >= 3, else all
times (:75-87); a missing cell falls back to a uniformly chosen view that has that time -- the intent of :98-107, whose
`time_caminfos[time_caminfos is not None]` keeps the None entries -- and raises ValueError when there is none.  Randomness comes from the
`rng` (a numpy Generator) given at construction, not from numpy's global state.  A camera keeps the RAW view_id / time_id of its record,
as the reference's Camera does.  On `device="cpu"` the same results come from composed torch operations (host-logic tests); on a GPU
there is only the kernel."""
from types import SimpleNamespace

import numpy as np
import torch

from . import native as _n

STORAGES = {"uint8": 0, "float32": 1}          # include/csplat.h: CSPLAT_CAMERA_UINT8, CSPLAT_CAMERA_FLOAT32
PITCH_ALIGN = 16                               # bytes: every stored plane begins on a multiple of it
_RING = 8                                      # pinned index buffers in flight
_RING_WORDS = 64
_UPLOADED_MAX = 4096                           # index sets kept on the device


def _bits(t):
    return t.contiguous().view(torch.int32)


def quantise_image(x):
    """the 8-bit levels u of a float32 image with u / 255.0 == x bit for bit (round(x * 255) / 255 == x), or None"""
    q = torch.round(x * 255.0)
    if not bool(((q >= 0) & (q <= 255)).all()):
        return None
    u = q.to(torch.uint8)
    return u if torch.equal(_bits(u / 255.0), _bits(x)) else None


def quantise_mask(m):
    """the 8-bit levels u of a float32 mask with 1.0 - u / 255.0 == m bit for bit (u = round((1 - m) * 255)), or None"""
    q = torch.round((1.0 - m) * 255.0)
    if not bool(((q >= 0) & (q <= 255)).all()):
        return None
    u = q.to(torch.uint8)
    return u if torch.equal(_bits(1.0 - u / 255.0), _bits(m)) else None


class CameraBatch(list):
    """the cameras of one step, in order; `gt` [n,3,H,W] and `mask` [n,1,H,W] (None without masks) are the tensors they are slices of,
    `slots` the store slots they were gathered from"""
    gt = mask = None
    slots = ()


class CameraDataset:
    def __init__(self, infos=(), args=None, device="cuda", storage="auto", rng=None, capacity=16):
        if storage not in ("auto",) + tuple(STORAGES):
            raise ValueError(f"CameraDataset: storage is 'auto', 'uint8' or 'float32', got {storage!r}")
        self.args = args
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.storage_request = storage
        self.storage = None if storage == "auto" else storage          # decided by the first frames under "auto"
        self.rng = rng if rng is not None else np.random.default_rng()
        self.size = None                       # (H, W) of every image
        self.has_mask = None
        self.n_slots = 0
        self.capacity = 0
        self._first_capacity = max(int(capacity), 1)
        self._store = None                     # uint8 [capacity * planes * pitch]
        self._pitch = 0
        self._wv = self._fp = self._cc = None  # per-slot tables: world_view_transform, full_proj_transform, camera_center
        self._views = {}                       # slot -> the three table rows as tensors (created once per slot and table)
        self._records = []                     # slot -> host-side fields of the camera
        self._slot_of = {}                     # (raw view id, raw time id) -> slot
        self._times = set()
        self._plan = None
        self._ring = None
        self._ring_at = 0
        self._uploaded = {}                    # slots of a step -> their int32 device array (slot numbers never change meaning)
        self.viewpoint_ids = np.zeros(0, np.int64)
        self.time_ids = np.zeros(0, np.int64)
        self.times = np.zeros(0)
        self.n_viewpoints = self.n_times = 0
        self._grid = np.zeros((0, 0), np.int64)
        self.uploaded_cells = 0                # cells uploaded since construction (re-uploads of replace=True included)
        if len(infos):
            self.add_frames(infos)

    # ---- the store ----------------------------------------------------------------------------------------------------------------
    @property
    def planes(self):
        return 3 + int(bool(self.has_mask))

    def _pitch_of(self, storage):
        hw = self.size[0] * self.size[1]
        return max(-(-hw * (4 if storage == "float32" else 1) // PITCH_ALIGN) * PITCH_ALIGN, PITCH_ALIGN)

    def _grow(self, need):
        if need <= self.capacity:
            return
        cap = max(self.capacity, self._first_capacity)
        while cap < need:
            cap *= 2
        per = self.planes * self._pitch
        store = torch.zeros(cap * per, dtype=torch.uint8, device=self.device)
        tables = [torch.zeros((cap,) + shape, dtype=torch.float32, device=self.device) for shape in ((4, 4), (4, 4), (3,))]
        if self.n_slots:
            store[:self.n_slots * per].copy_(self._store[:self.n_slots * per])
            for new, old in zip(tables, (self._wv, self._fp, self._cc)):
                new[:self.n_slots].copy_(old[:self.n_slots])
        self._store, (self._wv, self._fp, self._cc) = store, tables
        self._views = {}
        self.capacity = cap

    def _to_float32(self):
        """the uint8 store rewritten as float32 words: the values every step returned so far, bit for bit"""
        if self.n_slots:
            gt, mask = self._gather(list(range(self.n_slots)))
        self.storage, self._pitch = "float32", self._pitch_of("float32")
        hw = self.size[0] * self.size[1]
        store = torch.zeros(self.capacity * self.planes * self._pitch, dtype=torch.uint8, device=self.device)
        if self.n_slots:
            words = store.view(torch.float32).view(self.capacity, self.planes, self._pitch // 4)
            words[:self.n_slots, :3, :hw] = gt.view(self.n_slots, 3, hw)
            if self.has_mask:
                words[:self.n_slots, 3, :hw] = mask.view(self.n_slots, hw)
        self._store = store

    def _packed(self, frames, storage):
        """host bytes [k, planes, pitch] of (image, mask, levels of the image, levels of the mask) frames"""
        hw, pitch = self.size[0] * self.size[1], self._pitch_of(storage)
        out = torch.zeros(len(frames), self.planes, pitch, dtype=torch.uint8)
        words = out.view(torch.float32) if storage == "float32" else None
        for k, (img, msk, img8, msk8) in enumerate(frames):
            if storage == "float32":
                words[k, :3, :hw] = img.reshape(3, hw)
                if self.has_mask:
                    words[k, 3, :hw] = msk.reshape(hw)
            else:
                out[k, :3, :hw] = img8.reshape(3, hw)
                if self.has_mask:
                    out[k, 3, :hw] = msk8.reshape(hw)
        return out

    def add_frames(self, infos, replace=False):
        """upload the CameraInfo records (csplat/scene_io.py) whose (view_id, time_id) cell is not in the store yet -- with replace=True
        also those that are, over their slot -- and re-order the grid.  -> the number of cells uploaded.  ValueError, before anything
        changes: images of more than one size, records with and without a mask, an image or mask that is not float-like [3,H,W] /
        [1,H,W], storage="uint8" on data that is not exactly 8-bit levels over 255.  Of two records of one cell in `infos` the first
        is kept (the last with replace=True).  A truncation (`truncate_times`) and a `plan` end here."""
        from .synthetic import camera_matrices
        infos = list(infos)
        size, has_mask = self.size, self.has_mask
        for info in infos:
            if not torch.is_tensor(info.image) or info.image.dim() != 3 or info.image.shape[0] != 3:
                raise ValueError(f"CameraDataset: an image is a [3,H,W] tensor, got {getattr(info.image, 'shape', type(info.image).__name__)}")
            hw = (int(info.image.shape[1]), int(info.image.shape[2]))
            if size is None:
                size, has_mask = hw, info.mask is not None
            if hw != size:
                raise ValueError(f"CameraDataset: all images must be one size, got {hw} beside {size}")
            if (info.mask is not None) != has_mask:
                raise ValueError("CameraDataset: all records carry a mask or none does")
            if info.mask is not None and (not torch.is_tensor(info.mask) or info.mask.numel() != hw[0] * hw[1]):
                raise ValueError(f"CameraDataset: a mask is a [1,H,W] tensor of the image's size, got {getattr(info.mask, 'shape', None)}")
        todo = {}
        for info in infos:
            key = (int(info.view_id), int(info.time_id))
            if replace or (key not in self._slot_of and key not in todo):
                todo[key] = info
        frames, exact = [], True
        want8 = self.storage != "float32"
        for info in todo.values():
            img = info.image.clamp(0.0, 1.0).to(dtype=torch.float32, device="cpu")          # what camera_from_info makes of it
            msk = None if info.mask is None else info.mask.to(dtype=torch.float32, device="cpu")
            img8 = quantise_image(img) if want8 and exact else None
            msk8 = quantise_mask(msk) if want8 and exact and msk is not None and img8 is not None else None
            if want8 and (img8 is None or (msk is not None and msk8 is None)):
                if self.storage_request == "uint8":
                    raise ValueError(f"CameraDataset: storage='uint8', but {info.image_name!r} (view {info.view_id}, time {info.time_id}) is "
                                     "not 8-bit levels over 255 exactly")
                exact = False
            frames.append((img, msk, img8, msk8))
        # ---- nothing was changed so far
        self.size, self.has_mask = size, has_mask
        self._plan = None
        if frames:
            if self.storage is None:                                   # "auto": the first frames decide
                self.storage = "uint8" if exact else "float32"
            elif self.storage == "uint8" and not exact:                # "auto": later frames are not exact levels
                self._to_float32()
            if not self._pitch:
                self._pitch = self._pitch_of(self.storage)
            fresh = [k for k in todo if k not in self._slot_of]
            self._grow(self.n_slots + len(fresh))
            packed = self._packed(frames, self.storage)
            per = self.planes * self._pitch
            slots, nxt = [], self.n_slots
            for key in todo:
                s = self._slot_of.get(key)
                if s is None:
                    s, nxt = nxt, nxt + 1
                    self._slot_of[key] = s
                    self._records.append(None)
                slots.append(s)
            wv, fp, cc = [], [], []
            for s, info in zip(slots, todo.values()):
                a, b, c = camera_matrices(np.asarray(info.R), np.asarray(info.T), info.FovX, info.FovY)
                wv.append(a), fp.append(b), cc.append(c)
                self._records[s] = SimpleNamespace(uid=info.uid, FoVx=info.FovX, FoVy=info.FovY, time=float(info.time), view_id=info.view_id,
                                                   time_id=info.time_id, image_name=info.image_name)
                self._times.add(float(info.time))
            at = torch.as_tensor(slots, dtype=torch.int64, device=self.device)
            contiguous = slots == list(range(slots[0], slots[0] + len(slots)))
            for table, rows in ((self._wv, wv), (self._fp, fp), (self._cc, cc)):
                rows = torch.from_numpy(np.stack(rows).astype(np.float32)).to(self.device)
                if contiguous:
                    table[slots[0]:slots[0] + len(slots)].copy_(rows)
                else:
                    table[at] = rows
            if contiguous:           # (the fresh cells of a growing scene: one copy)
                self._store[slots[0] * per:(slots[0] + len(slots)) * per].copy_(packed.view(-1))
            else:
                for k, s in enumerate(slots):
                    self._store[s * per:(s + 1) * per].copy_(packed[k].view(-1))
            self.n_slots = nxt
            self.uploaded_cells += len(slots)
        self._order()
        return len(frames)

    def _order(self):
        """the view x time grid of slots (-1: no such cell): positions in the sorted unique ids (dataset.py:54-71)"""
        keys = list(self._slot_of)
        self.viewpoint_ids = np.unique(np.asarray([k[0] for k in keys], np.int64))
        self.time_ids = np.unique(np.asarray([k[1] for k in keys], np.int64))
        self.times = np.unique(np.asarray(sorted(self._times), np.float64))
        self.n_viewpoints, self.n_times = len(self.viewpoint_ids), len(self.time_ids)
        self._grid = np.full((self.n_viewpoints, self.n_times), -1, np.int64)
        for (v, t), s in self._slot_of.items():
            self._grid[np.searchsorted(self.viewpoint_ids, v), np.searchsorted(self.time_ids, t)] = s

    def truncate_times(self, n_times):
        """keep the first n_times columns of the grid: the `ordered_data[:, :n_times]` of the reference's update_data
        (train_utils.py:400-402).  Nothing leaves the store; the next add_frames orders the whole grid again."""
        if not 0 < int(n_times) <= self._grid.shape[1]:
            raise ValueError(f"CameraDataset.truncate_times: n_times lies in 1 .. {self._grid.shape[1]}, got {n_times}")
        self._grid = self._grid[:, :int(n_times)]
        self.n_times = int(n_times)
        self._plan = None

    # ---- the grid rules -----------------------------------------------------------------------------------------------------------
    def __len__(self):
        return self.n_viewpoints

    def slot(self, view, time):
        """the store slot of grid cell (view, time); a missing cell: that of a uniformly chosen view that has the time"""
        if not (0 <= int(view) < self.n_viewpoints and 0 <= int(time) < self.n_times):
            raise IndexError(f"CameraDataset: cell ({view}, {time}) is outside the {self.n_viewpoints} x {self.n_times} grid")
        s = int(self._grid[int(view), int(time)])
        if s < 0:
            have = np.nonzero(self._grid[:, int(time)] >= 0)[0]
            if not len(have):
                raise ValueError("No cam info found, this should not happen. Something is wrong in the provided data.")
            s = int(self._grid[have[int(self.rng.integers(len(have)))], int(time)])
        return s

    def item_times(self, view=None):
        """the time positions of __getitem__: (m - 1, m, m + 1) with m uniform in [1, n_times - 2] when n_times >= 3, else all"""
        if self.n_times >= 3:
            m = int(self.rng.integers(1, self.n_times - 1))
            return [m - 1, m, m + 1]
        return list(range(self.n_times))

    def __getitem__(self, view):
        return self.step(view, self.item_times(view))

    def get_one_item(self, view, time):
        return self.step(view, [time])[0]

    # ---- a step -------------------------------------------------------------------------------------------------------------------
    def plan(self, schedule):
        """upload the slot indices of a whole schedule, a list of (view, time_ids), once: the steps that follow IN THAT ORDER upload
        nothing.  A step that does not match the next planned entry is served the usual way and leaves the plan where it is.  Missing
        cells are resolved here (the rng is consumed in schedule order, as the same steps without a plan would consume it)."""
        keys, slots, offs = [], [], []
        for view, time_ids in schedule:
            keys.append((int(view), tuple(int(t) for t in time_ids)))
            offs.append(len(slots))
            slots += [self.slot(view, t) for t in time_ids]
        dev = torch.tensor(slots, dtype=torch.int32).to(self.device) if slots else torch.zeros(0, dtype=torch.int32, device=self.device)
        self._plan = SimpleNamespace(keys=keys, slots=slots, offs=offs, dev=dev, at=0)

    def _upload(self, slots):
        """the slot indices on the device, through a ring of small pinned buffers (an entry is reused once its copy has run)"""
        n = len(slots)
        if self.device.type != "cuda":
            return None
        if n > _RING_WORDS:
            return torch.tensor(slots, dtype=torch.int32).to(self.device)
        with _n.on_device(self.device):
            if self._ring is None:
                self._ring = [(torch.zeros(_RING_WORDS, dtype=torch.int32).pin_memory(), torch.cuda.Event()) for _ in range(_RING)]
            host, done = self._ring[self._ring_at]
            self._ring_at = (self._ring_at + 1) % _RING
            done.synchronize()
            host.numpy()[:n] = slots
            dev = torch.empty(n, dtype=torch.int32, device=self.device)
            dev.copy_(host[:n], non_blocking=True)
            done.record()
        return dev

    def _gather(self, slots, idx_dev=None):
        """(gt [n,3,H,W], mask [n,1,H,W] or None) of the given store slots: one launch on a GPU, composed torch on the CPU"""
        n, (H, W) = len(slots), self.size
        for s in slots:
            if not 0 <= s < self.n_slots:
                raise IndexError(f"CameraDataset: slot {s} is outside the store's {self.n_slots}")
        if self.device.type == "cuda":
            gt = torch.empty(n, 3, H, W, dtype=torch.float32, device=self.device)
            mask = torch.empty(n, 1, H, W, dtype=torch.float32, device=self.device) if self.has_mask else None
            if n and idx_dev is None:      # an index set seen before is on the device already (a run cycles through views x time triples)
                idx_dev = self._uploaded.get(tuple(slots))
                if idx_dev is None:
                    if len(self._uploaded) >= _UPLOADED_MAX:
                        self._uploaded.clear()
                    idx_dev = self._uploaded[tuple(slots)] = self._upload(slots)
            if n:
                _n.launch("csplat_camera_batch", self.device, n, H, W, STORAGES[self.storage], int(self.has_mask), self.n_slots, self._pitch,
                          _n.ptr(self._store), _n.ptr(idx_dev), _n.ptr(gt), _n.ptr(mask))
            return gt, mask
        _n.composed_fallback("camera_dataset.step", "mode", self._store)
        rows = self._store.view(self.capacity, self.planes, self._pitch)[torch.as_tensor(slots, dtype=torch.int64)]
        if self.storage == "uint8":
            rows = rows[:, :, :H * W]
            gt = (rows[:, :3] / 255.0).reshape(n, 3, H, W)
            mask = (1.0 - rows[:, 3:] / 255.0).reshape(n, 1, H, W) if self.has_mask else None
        else:
            rows = rows.contiguous().view(torch.float32)[:, :, :H * W]
            gt = rows[:, :3].reshape(n, 3, H, W).clone()
            mask = rows[:, 3:].reshape(n, 1, H, W).clone() if self.has_mask else None
        return gt, mask

    def _rows(self, s):
        v = self._views.get(s)
        if v is None:
            v = self._views[s] = (self._wv[s], self._fp[s], self._cc[s])
        return v

    def step(self, view, time_ids):
        """the cameras (view, t) for t in time_ids as a CameraBatch: ONE launch.  IndexError for a cell outside the grid, before
        anything is launched."""
        key = (int(view), tuple(int(t) for t in time_ids))
        p, idx_dev = self._plan, None
        if p is not None and p.at < len(p.keys) and p.keys[p.at] == key:
            off = p.offs[p.at]
            slots = p.slots[off:off + len(key[1])]
            idx_dev = p.dev[off:off + len(key[1])]
            p.at += 1
        else:
            slots = [self.slot(view, t) for t in key[1]]
        gt, mask = self._gather(slots, idx_dev)
        H, W = self.size
        batch = CameraBatch()
        batch.gt, batch.mask, batch.slots = gt, mask, tuple(slots)
        images, masks = gt.unbind(0), (None,) * len(slots) if mask is None else mask.unbind(0)          # (one call each, not one per camera)
        for i, s in enumerate(slots):
            r, (wv, fp, cc) = self._records[s], self._rows(s)
            batch.append(SimpleNamespace(uid=r.uid, image_height=H, image_width=W, FoVx=r.FoVx, FoVy=r.FoVy, world_view_transform=wv,
                                         full_proj_transform=fp, camera_center=cc, time=r.time, original_image=images[i],
                                         mask=masks[i], view_id=r.view_id, time_id=r.time_id,
                                         image_name=r.image_name, gt_stack=gt, gt_index=i, mask_stack=mask))
        return batch


MDNerfDataset = CameraDataset
