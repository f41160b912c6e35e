"""Z-slab partition of one TSDF volume over the GPUs of a node.

One process per GPU, `torch.distributed` (backend "nccl" == RCCL over xGMI on ROCm).  The reference has
no multi-GPU path at all; what is partitioned here is the reference's single volume:

  * K1 (integrate) shards by voxels: rank g owns Z planes [z0_g, z1_g) -- no communication.
  * brick occupancy (K6) is replicated: every rank marks all bricks from the (replicated) frame images;
    2 atomics per depth pixel are cheaper than any collective.
  * K2 needs the voxels just across a slab face (trilinear + gradient taps).  Either each rank's boundary tile layers
    are all-gathered and the neighbours' faces land in the local halo (halo="exchange"), or every rank simply integrates
    its halo layers itself (halo="recompute": K1's voxels are independent, one extra tile layer per face costs less than
    any collective).
  * every rank steps the SAME global ray (identical fp32 position sequence) and samples only the
    positions inside its slab; the partial results are gathered on rank 0 -- as full images (composite="dense") or as
    one 32-byte record per hit ray (composite="compact") -- and the hit with the smallest sample count wins, which is
    exactly the single-GPU first zero crossing.
  * K3/K4 (hole filling) are image space and tiny: rank 0 only.
  * compositor="dedicated": rank 0 holds NO slab.  The image-space tail of a frame on the gathering rank (receive, composite, hole
    filling: ~70 us at 1280x720) is longer than a slab's share of the volume work at any of the BASELINE configurations, so with an
    even split rank 0 is the frame's critical path and the other ranks wait for it in every gather.  With a dedicated compositor the
    volume is split over ranks 1 .. N-1 and rank 0 only receives, composites and fills: while it finishes frame f the workers are
    already integrating frame f + 1 (each rank's work is queued on its stream; the gather is the only meeting point), and the frame
    period is max(worker, compositor) instead of their sum.  With the compact composite the compositor does not march, so the
    write-only diagnostic image of sample counts (tex_num_samples, recon_integration.cpp:207-209: cleared and bound for imageStore,
    read by nothing) holds 0 at the pixels no exported ray covers instead of the ray's total sample count; colour, depth, the sample counts of
    hit pixels and the hole-filled framebuffer are those of the single-GPU frame, bit for bit.

The exchange works on plain device pointers across the C ABI (tsdf_halo_*_dev, tsdf_export_partial_dev,
tsdf_composite_dev); torch only owns the buffers and the collective.

Stream order.  The backend's kernels and torch's collectives must share ONE stream: the driver creates an explicit
`torch.cuda.Stream`, hands its (non-zero) handle to the backend and issues every collective under
`torch.cuda.stream(...)`.  (torch's default stream has the handle 0, which `tsdf_set_stream` reads as "back to the
context's own stream": a driver that passed it left the kernels on a private non-blocking stream, unordered against the
collectives.  binding.set_stream now maps 0 to tsdf_adopt_null_stream, and this driver does not rely on it.)

No host synchronisation per frame.  The compact composite gathers a FIXED number of records per rank, decided from the
all-gathered hit counts of the frame `LAG` frames earlier (identical on every rank, read from a pinned copy whose event
completed long ago) times 1.5.  A frame whose slab hit more rays than that is detected from the same counts: `finish()`
-- the call that precedes any read of the result -- re-exports and re-gathers that frame with the exact size, so results
never depend on the guess.  All ranks see the same counts, so they take the same decision at the same frame.
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch
import torch.distributed as dist

from .slab_exchange import NONE, GatherBook, SlabRoles
from .binding import (MESH_COMPONENT_DTYPE, MESH_SEAM_ROOT_DTYPE, MESH_SEAM_VERTEX_DTYPE, RAY_HIT_DTYPE, RAY_SURFACE_DTYPE, as_rays, join_mesh_parts,
                      merge_mesh_component_seams, merge_ray_parts)


def worker_slab_range(res_z: int, rank: int, world: int):
    """Slab of rank `rank` when rank 0 is a dedicated compositor: ranks 1 .. world-1 split the volume; rank 0 gets the first worker's
    slab as a placeholder (its context needs SOME valid volume -- a slab may not be thinner than its halo --; it is never integrated
    or marched)."""
    return slab_range(res_z, max(rank - 1, 0), world - 1)


def balanced_slab_ranges(layer_weights, world: int, res_z: int):
    """Contiguous tile-aligned split of the Z axis into `world` slabs of about equal total weight (every slab at least one tile layer):
    the occupied bricks of a scene are not spread evenly over z, and the frame period of the partition is its slowest slab's.
    `layer_weights[l]` is the cost of tile layer l (e.g. its occupied bricks plus a constant for the per-layer floor); every rank
    must pass the same weights.  Returns [(z0, z1)] in voxel planes."""
    w = [float(x) for x in layer_weights]
    layers = len(w)
    assert layers == (res_z + 7) // 8 and 1 <= world <= layers
    cum = [0.0]
    for x in w:
        cum.append(cum[-1] + x)
    bounds = [0]
    for k in range(1, world):
        target = cum[-1] * k / world
        b = bounds[-1] + 1
        while b < layers and cum[b] < target:
            b += 1
        if b > bounds[-1] + 1 and abs(cum[b - 1] - target) <= abs(cum[b] - target):
            b -= 1                                       # the boundary nearest to the target
        b = max(bounds[-1] + 1, min(b, layers - (world - k)))
        bounds.append(b)
    bounds.append(layers)
    return [(bounds[k] * 8, min(bounds[k + 1] * 8, res_z)) for k in range(world)]


def slab_range(res_z: int, rank: int, world: int):
    """Tile-aligned (8 planes) contiguous split of the Z axis; the last rank takes the remainder."""
    layers = (res_z + 7) // 8
    base, extra = divmod(layers, world)
    lo = rank * base + min(rank, extra)
    hi = lo + base + (1 if rank < extra else 0)
    return lo * 8, min(hi * 8, res_z)


class SlabDriver:
    """Runs the per-frame call order of source/kinect_client.cpp:569-599,614 on one slab.

    `backend` is a ReconIntegrationHip created with slab=slab_range(...) (tests inject a stand-in with the same hook
    methods).  `buf_device` is where exchange buffers live ("cuda:N"; "cpu" for the stand-in); with a gloo group and
    CUDA buffers the collective is staged through host memory.

    halo       "exchange": all-gather of the boundary tile layers before the raymarch (the backend must NOT have been
               created with recompute_halo); "recompute": the backend integrates its own halo layers, no collective.
    composite  "dense": every rank ships 24 B per view pixel to rank 0; "compact": one 32-byte record per ray that hit in
               the slab, a fixed number per rank and frame (see the module docstring).
    exchange_when_alone   world == 1 normally draws the frame directly; True runs the whole exchange (pack, collectives, composite)
               with the one rank anyway -- used to drive the RCCL calls on a box with a single GPU.
    stream     the torch stream everything runs on (default: a new one).  CUDA buffers only.
    min_capacity  smallest number of hit records gathered per rank (compact composite).
    compositor "shared": every rank owns a slab, rank 0 composites as well; "dedicated" (world >= 2): rank 0 owns no slab -- its
               backend only needs the view (worker_slab_range() gives the workers' slabs) -- and never integrates or marches.
    """

    LAG = GatherBook.LAG   # frames between a hit count and its use as the gather size: its pinned copy has long arrived, the host never waits

    def __init__(self, backend, rank, world, buf_device, group=None, view=(1280, 720), halo="exchange", composite="dense", preprocess=False,
                 exchange_when_alone=False, stream=None, min_capacity=4096, compositor="shared", native=False, max_capacity=0):
        """native: the two exchanges run inside the library (tsdf_halo_exchange / tsdf_composite_gather / tsdf_composite_finish, comm.cpp: RCCL
        called from C++ on the context's stream) and this class only issues the frame's calls -- what a C++ host does; torch.distributed is
        then used once, to carry the communicator's 128-byte id from rank 0 to the others.  Compact composite only."""
        assert halo in ("exchange", "recompute") and composite in ("dense", "compact") and compositor in ("shared", "dedicated")
        self.native = bool(native)
        assert not self.native or composite == "compact", "the native exchange gathers hit records (compact composite)"
        assert compositor == "shared" or world >= 2, "a dedicated compositor needs at least one worker rank"
        self.dedicated = compositor == "dedicated"
        self.roles = SlabRoles(rank, world, self.dedicated)          # who owns a slab, exports, which halo rows are its neighbours (slab_exchange.py)
        self.is_worker, self.first_worker = self.roles.worker, self.roles.first_worker
        self.b, self.rank, self.world, self.dev, self.group = backend, rank, world, torch.device(buf_device), group
        self.view, self.halo, self.composite = view, halo, composite
        self.preprocess = preprocess          # frames start from the raw sensor images: processTextures() instead of markBricks()
        self.exchanging = world > 1 or exchange_when_alone
        self.stage_cpu = self.exchanging and not self.native and dist.get_backend(group) == "gloo" and self.dev.type == "cuda"
        # the collectives are torch's, so the context's kernels go to a torch stream -- but only when there IS an exchange: a context that
        # keeps its own stream has its three lanes (stage overlap) on consecutively created streams, i.e. on different hardware queues
        self.stream = None
        if self.dev.type == "cuda" and self.exchanging and not self.native:
            self.stream = stream if stream is not None else torch.cuda.Stream(self.dev)
            assert self.stream.cuda_stream != 0, "the NULL stream cannot be handed to tsdf_set_stream"
            backend.set_stream(self.stream.cuda_stream)
        # The compact composite's frame bookkeeping -- capacities, ring slots, repairs, verdicts, the two statistics -- is the book's (slab_exchange.py,
        # the twin of the library's).  No maximum here: max_capacity bounds the NATIVE exchange's guess only (recorded behaviour)
        self.book = GatherBook(min_capacity)
        self.last = None                      # a compact frame is pending until finish() has checked it
        if self.exchanging and self.native:
            ids = [backend.comm_unique_id() if rank == 0 else None]
            if world > 1:
                dist.broadcast_object_list(ids, src=0, group=group)
            with self._on_stream():
                backend.comm_init(ids[0], rank, world, dedicated_compositor=self.dedicated)
                backend.comm_set_capacity_limits(int(min_capacity), max_capacity)
            self.stage_cpu = False
        elif self.exchanging:
            npx = view[0] * view[1]
            self.npx = npx
            with self._on_stream():
                if halo == "exchange":
                    layers, nbytes = backend.halo_info()
                    n = nbytes // 4
                    self.send = torch.empty((2, n), dtype=torch.float32, device=self.dev)
                    self.gath = torch.empty((world, 2, n), dtype=torch.float32, device=self.dev)
                if composite == "dense":
                    # 24 B / pixel; a compositor without a slab contributes "no hit, no samples" for every pixel (sample count 0)
                    self.part = (torch.empty if self.is_worker else torch.zeros)(npx * 6, dtype=torch.float32, device=self.dev)
                    self.parts = torch.empty((world, npx * 6), dtype=torch.float32, device=self.dev) if rank == 0 else None
                else:
                    self.hitbuf = torch.zeros(8 + npx * 8, dtype=torch.float32, device=self.dev)     # 32 B header + 32 B records; a slab cannot hit more rays than there are pixels
                    self.hitparts = torch.zeros((world, 8 + npx * 8), dtype=torch.float32, device=self.dev) if rank == 0 else None
                    self.counts = torch.zeros((world, 2), dtype=torch.int32, device=self.dev)        # per rank: [records written, rays hit]
                    self.counts_host = [torch.zeros((world, 2), dtype=torch.int32, pin_memory=(self.dev.type == "cuda")) for _ in range(GatherBook.RING)]
                    self.counts_evt = [None] * GatherBook.RING
            if self.stream is not None:
                self.stream.synchronize()

    # frames gathered by the torch path; frames finish() repaired / frames left truncated (native: refreshed from the library's by finish())
    frame_no = property(lambda self: self.book.frame_no)
    regathers = property(lambda self: self.book.regathers)
    overflowed_frames = property(lambda self: self.book.overflowed_frames)

    # ------------------------------------------------------------------ plumbing
    def _on_stream(self):
        return torch.cuda.stream(self.stream) if self.stream is not None else contextlib.nullcontext()

    def _all_gather(self, out, inp):
        if self.stage_cpu:
            o = torch.empty(out.numel(), dtype=out.dtype)
            dist.all_gather_into_tensor(o, inp.reshape(-1).cpu(), group=self.group)
            out.view(-1).copy_(o)
        else:
            dist.all_gather_into_tensor(out.view(-1), inp.reshape(-1), group=self.group)

    def _gather0(self, out_rows, inp):
        """gather `inp` (1-D) of every rank into out_rows[r] (1-D views of equal length) on rank 0"""
        if self.stage_cpu:
            lst = [torch.empty(inp.shape, dtype=inp.dtype) for _ in range(self.world)] if self.rank == 0 else None
            dist.gather(inp.cpu(), lst, dst=0, group=self.group)
            if self.rank == 0:
                for row, t in zip(out_rows, lst):
                    row.copy_(t)
        else:
            dist.gather(inp, out_rows if self.rank == 0 else None, dst=0, group=self.group)

    def exchange_halo(self):
        b = self.b
        if self.is_worker:
            b.halo_pack_dev(self.send[0].data_ptr(), self.send[1].data_ptr())
        self._all_gather(self.gath, self.send)
        if not self.is_worker:
            return                                                   # (took part in the collective; has no slab faces of its own)
        lo, hi = self.roles.below(), self.roles.above()              # the lower neighbour's HIGH face, the upper neighbour's LOW face
        b.halo_unpack_dev(self.gath[lo].data_ptr() if lo[0] != NONE else 0, self.gath[hi].data_ptr() if hi[0] != NONE else 0)

    # ------------------------------------------------------------------ compact composite: sizes without a host sync
    def _max_hits(self, slot):
        """the largest per-rank hit count among the all-gathered [written, hit] counts in ring slot `slot` (waits for their pinned copy: for a frame
        LAG frames back it arrived long ago)"""
        if self.counts_evt[slot] is not None:
            self.counts_evt[slot].synchronize()
        return int(self.counts_host[slot][:, 1].max())

    def _capacity(self, f):
        """records gathered per rank for frame f, the one about to be gathered: 1.5 x the largest per-rank hit count of frame f - LAG (the same
        number on every rank)"""
        slot = self.book.lagged_slot()
        return self.book.open(self.npx, self._max_hits(slot) if slot != NONE else 0)

    def frame_status(self, f):
        """True: frame f (counted from 0) of the compact composite was built from truncated record lists and not repaired -- a caller that kept
        that frame must redraw it.  Known at once for the latest LAG + 1 frames (waits for their counts), from the last 64 verdicts otherwise;
        KeyError: not gathered yet / too old.  (tsdf_comm_frame_status is the same rule inside the library.)"""
        if self.exchanging and self.native:
            return self.b.comm_frame_status(f)
        kind, truncated, slot, cap = self.book.status(f)
        if kind == GatherBook.VERDICT:
            return bool(truncated)
        if kind == GatherBook.COMPARE:
            return self._max_hits(slot) > cap
        raise KeyError(f"no verdict for frame {f} ({self.frame_no} frames gathered)")

    def _exchange_hits(self, cap, first):
        """first: the frame's first exchange, which also all-gathers the hit counts; False on a repeated one (finish()).  Rank 0's own records never
        travel: it exports them -- ALL of them, whatever the capacity of the gather -- straight into its row of the gather buffer, once
        per frame (a repeated gather must not export them again: the first composite has overwritten the march target they are read from)."""
        b, roles = self.b, self.roles
        own = self.hitparts[0] if roles.own_in_parts else self.hitbuf
        if roles.exports(first):
            b.export_hits_dev(own.data_ptr(), roles.export_records(self.npx, cap))     # (a compositor's header stays {0 records, 0 hits})
        if first:
            self._all_gather(self.counts, own[:2].view(torch.int32))
            slot = self.book.open_slot()
            self.counts_host[slot].copy_(self.counts, non_blocking=True)
            if self.stream is not None:
                ev = self.counts_evt[slot] or torch.cuda.Event()
                ev.record(self.stream)
                self.counts_evt[slot] = ev
        n = roles.exchange_floats(cap)
        if roles.grouped:       # (rank 0's contribution to the collective is a header-sized dummy: its row is in place already)
            if self.rank == 0 and getattr(self, "selfrow", None) is None:
                self.selfrow = torch.zeros_like(self.hitbuf)
            self._gather0([self.selfrow[:n]] + [self.hitparts[r, :n] for r in range(1, self.world)] if self.rank == 0 else None, self.hitbuf[:n])
        if self.rank == 0:
            b.composite_hits_dev(self.hitparts.data_ptr(), self.world, self.hitparts.stride(0) * 4)
            b.fillColors()

    # ------------------------------------------------------------------ frame distribution ("ncclBroadcast from the receiving rank")
    def broadcast_frame(self, root, tensors=None):
        """The frame arrived on `root` (there: its four arrays as device tensors -- depth RG32F, quality, silhouette, colour RGB8 --, elsewhere
        None): every rank gets a copy and the ranks that own a slab re-lay it out.  native: tsdf_broadcast_frame (RCCL called from C++);
        else ONE torch.distributed broadcast of the packed arrays, then tsdf_upload_frame_dev."""
        with self._on_stream():
            if self.native:
                self.b.broadcast_frame(root, dev_ptrs=[t.data_ptr() for t in tensors] if self.rank == root else None)
                return
            n, (h, w, ch, cw) = self.b.n, self.b._dims
            npx, ncp = n * h * w, n * ch * cw
            offs = (0, npx * 8, npx * 12, npx * 16)
            if getattr(self, "frame_stage", None) is None:
                self.frame_stage = torch.empty(npx * 16 + ((ncp * 3 + 15) // 16) * 16, dtype=torch.uint8, device=self.dev)
            st = self.frame_stage
            if self.rank == root:
                for off, t in zip(offs, tensors):
                    b = t.contiguous().view(torch.uint8).reshape(-1)
                    st[off:off + b.numel()].copy_(b)
            if self.world > 1:
                if self.stage_cpu:
                    t = st.cpu()
                    dist.broadcast(t, src=root, group=self.group)
                    st.copy_(t)
                else:
                    dist.broadcast(st, src=root, group=self.group)
            if self.is_worker:
                p = st.data_ptr()
                self.b.upload_frame_dev(p + offs[0], p + offs[1], p + offs[2], p + offs[3])

    # ------------------------------------------------------------------ per frame
    def frame(self, mv, proj, new_frame=None):
        """new_frame: device pointers (depth_rg, quality, silhouette, colour) of a frame that has just arrived in device memory -- the
        ranks that own a slab re-lay it out first (tsdf_upload_frame_dev: what a new frame costs the path itself)"""
        with self._on_stream():
            self._frame(mv, proj, new_frame)

    def _frame(self, mv, proj, new_frame=None):
        b = self.b
        if self.is_worker and not self.exchanging and not self.preprocess:   # one rank, nothing to exchange: the whole frame in one call into the library
            b.frame_dev(mv, proj, new_frame)
            return
        if self.is_worker and not self.exchanging and self.preprocess and new_frame is not None:   # ... and from the RAW frame (depth_raw, colour)
            b.frame_raw_dev(mv, proj, new_frame)
            return
        if self.is_worker and new_frame is not None:
            if self.preprocess:
                b.upload_raw_frame_dev(*new_frame, complete=True)
            else:
                b.upload_frame_dev(*new_frame, complete=True)
        if self.is_worker:
            b.clearOccupiedBricks()
            if self.preprocess:
                b.processTextures()
            else:
                b.markBricks()
            b.updateOccupiedBricks(False)
            b.integrate()
        if not self.exchanging:
            b.drawF(mv, proj)
            return
        if self.native:
            if self.halo == "exchange":
                b.halo_exchange()
            if self.is_worker:
                b.draw(mv, proj)
            b.composite_gather()
            self.last = True
            return
        if self.halo == "exchange":
            self.exchange_halo()
        if self.is_worker:
            b.draw(mv, proj)
        if self.composite == "dense":
            if self.is_worker:
                b.export_partial_dev(self.part.data_ptr())
            self._gather0(list(self.parts.unbind(0)) if self.rank == 0 else None, self.part)
            if self.rank == 0:
                b.composite_dev(self.parts.data_ptr(), self.world)
                b.fillColors()
            return
        cap = self._capacity(self.frame_no)
        self._exchange_hits(cap, first=True)
        self.book.queued(cap)
        self.last = True

    # ------------------------------------------------------------------ the fused surface as ONE mesh, extracted where the volume is
    def extract_mesh(self, normals=True, colours=True, level=0):
        """A COLLECTIVE: every rank extracts its slab's part of the whole volume's mesh (tsdf_mesh_slab_extract; the halo must be current, as after
        frame()), the counts and the seam tables are all-gathered, every rank links its triangles with global indices, and the parts are gathered on
        rank 0.  Returns dict(part=the rank's arrays, vertex_base=..., counts=[world][2]) and, on rank 0, mesh=the concatenation: the arrays
        extract_mesh(level=...) of a whole-volume context gives.  A dedicated compositor contributes zero counts and an empty part."""
        b = self.b
        s = 8 << int(level)
        shape = (-(-int(b.res[1]) // s), -(-int(b.res[0]) // s))        # [nty][ntx] lattice tiles
        if self.is_worker:
            nv, nt = b.extract_mesh_slab(normals, colours, level)
            seam = np.asarray(b.mesh_slab_seam(), np.uint32).reshape(shape)
        else:
            nv, nt, seam = 0, 0, np.zeros(shape, np.uint32)
        world = self.world
        if world > 1:
            mine = torch.cat([torch.tensor([nv, nt], dtype=torch.int64), torch.from_numpy(seam.astype(np.int64).reshape(-1))]).to(self.dev)
            rows = torch.empty((world, mine.numel()), dtype=torch.int64, device=self.dev)
            with self._on_stream():
                self._all_gather(rows, mine)
                rows = rows.cpu().numpy()
        else:
            rows = np.concatenate([[nv, nt], seam.reshape(-1)]).astype(np.int64)[None]
        counts = rows[:, :2]
        base = int(counts[:self.rank, 0].sum())
        if self.is_worker:
            above = rows[self.rank + 1, 2:].astype(np.uint32).reshape(shape) if self.rank < world - 1 else None   # the slab above follows directly
            b.mesh_slab_link(base, above)
            part = b.mesh_slab_download(normals, colours)
        else:
            part = dict(position=np.zeros((0, 3), np.float32), triangles=np.zeros((0, 3), np.uint32))
            if normals:
                part["normal"] = np.zeros((0, 3), np.float32)
            if colours:
                part["colour"] = np.zeros((0, 4), np.float32)
        out = dict(part=part, vertex_base=base, counts=counts.copy())
        self._mesh_counts = counts.copy()                                # (mesh_components: every part's base and size)
        parts = [part]
        if world > 1:
            parts = [None] * world if self.rank == 0 else None
            dist.gather_object(part, parts, dst=0, group=self.group)
        if self.rank == 0:
            out["mesh"] = {k: np.concatenate([p[k] for p in parts]) for k in part}
        return out

    # ------------------------------------------------------------------ ... and its components, labelled where the parts are
    def mesh_components(self):
        """A COLLECTIVE, after extract_mesh: every rank labels its linked part alone (tsdf_mesh_slab_components), the three seam lists are all-gathered,
        every rank runs the same host merge (tsdf_mesh_merge_component_seams) and links its part (tsdf_mesh_slab_link_components), and the arrays are
        gathered on rank 0.  Returns dict(part=the rank's vertex_component / triangle_component / table, component_base, n_components) and, on rank 0,
        components=the concatenation: what mesh_components() + mesh_download_components() of a whole-volume context give for extract_mesh's mesh.
        A dedicated compositor contributes an empty part."""
        counts = getattr(self, "_mesh_counts", None)
        if counts is None:
            raise RuntimeError("mesh_components labels the parts of an extract_mesh: call that first")
        b = self.b
        mine = dict(vertex_base=int(counts[:self.rank, 0].sum()), n_vertices=int(counts[self.rank, 0]), n_local=0,
                    down=np.zeros(0, MESH_SEAM_VERTEX_DTYPE), up=np.zeros(0, MESH_SEAM_VERTEX_DTYPE), roots=np.zeros(0, MESH_SEAM_ROOT_DTYPE))
        if self.is_worker:
            mine["n_local"] = b.mesh_slab_components()["local_components"]
            mine.update(b.mesh_slab_component_seam())
        slabs = [mine]
        if self.world > 1:
            slabs = [None] * self.world
            dist.all_gather_object(slabs, mine, group=self.group)
        merged = merge_mesh_component_seams(slabs, native=True)
        if self.is_worker:
            b.mesh_slab_link_components(merged["component_base"][self.rank], merged["links"][self.rank])
            part = b.mesh_slab_download_components()
        else:
            part = dict(vertex_component=np.zeros(0, np.uint32), triangle_component=np.zeros(0, np.uint32), table=np.zeros(0, MESH_COMPONENT_DTYPE))
        out = dict(part=part, component_base=merged["component_base"][self.rank], n_components=merged["n_components"])
        parts = [part]
        if self.world > 1:
            parts = [None] * self.world if self.rank == 0 else None
            dist.gather_object(part, parts, dst=0, group=self.group)
        if self.rank == 0:
            out["components"] = {k: np.concatenate([p[k] for p in parts]) for k in part}
        return out

    # ------------------------------------------------------------------ ... and streamed every frame: tile-local parts that join unaided
    def stream_mesh(self, tag=0, take=True, wait=True):
        """Queue this rank's PART of the frame's mesh on its part ring (mesh_stream_config(part=True) on the backend first; the halo must be current,
        as after frame()): no exchange, no link step, no host wait -- a part is complete by itself.  take=False: that is all, the caller picks the
        frame up from the backend when it likes (mesh_stream_take).  take=True: a COLLECTIVE -- every rank takes its oldest part (waiting for it), the
        parts are gathered on rank 0 and joined by the header's rule; returns dict(part=the rank's (vertices, codes, info) or None) and, on rank 0,
        frame=(vertices, codes, info): the whole-volume compact frame, or None when a part overflowed (the frame is dropped whole).  A dedicated
        compositor contributes no part.  Part rings configured with taps=True carry each part's packed texture taps in info["taps"]; they travel with
        the part and the joined frame's info["taps"] is their concatenation, the whole-volume ring's block byte for byte."""
        if self.is_worker:
            self.b.mesh_stream(tag)
        if not take:
            return None
        part = self.b.mesh_stream_take(wait=wait) if self.is_worker else None
        parts = [part]
        if self.world > 1:
            parts = [None] * self.world if self.rank == 0 else None
            dist.gather_object(part, parts, dst=0, group=self.group)
        out = dict(part=part)
        if self.rank == 0:
            parts = [p for p in parts if p is not None]
            out["frame"] = None if any(p[2]["overflow"] for p in parts) else join_mesh_parts(parts)
        return out

    # ------------------------------------------------------------------ ray queries: every slab casts its part, rank 0 merges
    def cast_rays(self, rays, normals=False, colours=False, unit_cube=False):
        """A COLLECTIVE: every rank casts the SAME rays on its slab (tsdf_cast_rays_part_dev; the halo must be current, as after frame()), the parts go
        to rank 0 through the driver's gather, and rank 0 merges them on the device (tsdf_merge_ray_parts_dev).  Rank 0 returns what cast_rays of a
        whole-volume context gives -- hits, or (hits, surface) with normals or colours --, the other ranks None.  A dedicated compositor casts nothing
        and merges the workers' parts.  With host buffers (the tests' stand-in backend) the parts are cast and merged on the host by the same rule."""
        rays = as_rays(rays)
        n, want = len(rays), bool(normals or colours)
        rows, cuda = (2 if want else 1), self.dev.type == "cuda"
        with self._on_stream():
            mine = torch.zeros((rows, n, 32), dtype=torch.uint8, device=self.dev)      # [hit records][surface records]
            if self.is_worker and cuda:
                d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 32).copy()).to(self.dev)
                if self.stream is None:
                    torch.cuda.synchronize(self.dev)                     # the context runs on its own stream: the buffers must exist before it writes them
                self.b.cast_rays_part_dev(d_rays.data_ptr(), n, mine[0].data_ptr(), mine[1].data_ptr() if want else 0, normals, colours, unit_cube)
                if self.stream is None:
                    self.b.sync()
            elif self.is_worker:
                part = self.b.cast_rays_part(rays, normals=normals, colours=colours, unit_cube=unit_cube)
                for row, a in enumerate(part if want else (part,)):
                    mine[row] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(n, 32).copy())
            parts = mine[None]
            if self.world > 1:
                parts = torch.zeros((self.world, rows, n, 32), dtype=torch.uint8, device=self.dev) if self.rank == 0 else None
                self._gather0([parts[r].view(-1) for r in range(self.world)] if self.rank == 0 else None, mine.view(-1))
            if self.rank != 0:
                return None
            parts = parts[self.first_worker:]                            # (a compositor without a slab has no part)
            if cuda:                                                     # part k: its hit records, then its surface records -- rows * n records apart
                out = torch.zeros((rows, n, 32), dtype=torch.uint8, device=self.dev)
                if self.stream is None:
                    torch.cuda.synchronize(self.dev)
                self.b.merge_ray_parts_dev(parts[0, 0].data_ptr(), parts[0, 1].data_ptr() if want else 0, parts.shape[0], n, rows * n, out[0].data_ptr(),
                                           out[1].data_ptr() if want else 0)
                if self.stream is None:
                    self.b.sync()
                got = out.cpu().numpy()                                  # (on self.stream: behind the merge)
                hits = got[0].reshape(-1).view(RAY_HIT_DTYPE)
                return (hits, got[1].reshape(-1).view(RAY_SURFACE_DTYPE)) if want else hits
            got = parts.numpy()
            each = [(p[0].reshape(-1).view(RAY_HIT_DTYPE), p[1].reshape(-1).view(RAY_SURFACE_DTYPE)) if want else p[0].reshape(-1).view(RAY_HIT_DTYPE) for p in got]
            return merge_ray_parts(each)

    def pick(self, mv, proj, x, y, colours=True):
        """A COLLECTIVE: what is under pixel (x, y) of the view, as ReconIntegrationHip.pick -- the pixel's own ray (tsdf_view_rays needs no volume: every
        rank forms the same ray), then cast_rays.  Rank 0 returns pick()'s dict, the other ranks None."""
        ray = self.b.view_rays(mv, proj, (int(x), int(y), 1, 1))
        got = self.cast_rays(ray, normals=True, colours=colours, unit_cube=True)
        return None if got is None else self.b.pick_result(got[0][0], got[1][0])

    def finish(self):
        """Completes the latest frame: call before reading its result (and at the end of a timed region).  A COLLECTIVE when
        the compact gather of that frame turned out too small -- every rank sees the same counts and re-gathers together."""
        if self.exchanging and self.native:
            if self.last is not None:
                self.last = None
                with self._on_stream():
                    self.b.composite_finish()
                st = self.b.comm_stats()
                self.book.regathers, self.book.overflowed_frames = st["regathers"], st["overflowed_frames"]
        elif self.exchanging and self.composite == "compact" and self.last is not None:
            self.last = None
            regather, cap = self.book.finish(self.npx, self._max_hits(self.book.pending_slot()))
            if regather:
                with self._on_stream():
                    self._exchange_hits(cap, first=False)
        if self.stream is not None:
            self.stream.synchronize()
        elif hasattr(self.b, "sync"):
            self.b.sync()


def mesh_slabs_on_one_device(backends, normals=True, colours=True, level=0):
    """SlabDriver.extract_mesh with ONE visible device: backends[k] owns slab k (contiguous, in z order), each with a current halo (as
    frame_slabs_on_one_device leaves it).  Every slab extracts its part, the prefix of the counts gives each part's vertex base, each seam table goes
    one slab downwards, every slab links.  Returns the concatenated arrays -- the mesh extract_mesh(level=...) of a whole-volume context gives -- plus
    counts [(vertices, triangles)] and seams [table] per slab."""
    counts = [b.extract_mesh_slab(normals, colours, level) for b in backends]
    seams = [b.mesh_slab_seam() for b in backends]
    parts, base = [], 0
    for k, b in enumerate(backends):
        b.mesh_slab_link(base, seams[k + 1] if k + 1 < len(backends) else None)
        parts.append(b.mesh_slab_download(normals, colours))
        base += counts[k][0]
    out = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    out["counts"], out["seams"] = counts, seams
    return out


def mesh_components_on_one_device(backends, native=True):
    """SlabDriver.mesh_components with ONE visible device, after mesh_slabs_on_one_device on the same backends: every slab labels its linked part and
    exports its lists, the host merge runs once (native: the library's function, else its numpy twin), every slab links.  Returns the concatenated
    vertex_component, triangle_component and table -- what mesh_components() + mesh_download_components() of a whole-volume context give -- plus
    n_components, lists (the merge's input, per slab), merged (its output) and counts (mesh_slab_components() per slab)."""
    counts = [b.mesh_slab_components() for b in backends]
    lists, base = [], 0
    for b, n in zip(backends, counts):
        nv = b.mesh_slab_download(False, False, triangles=False)["position"].shape[0]
        lists.append(dict(vertex_base=base, n_vertices=nv, n_local=n["local_components"], **b.mesh_slab_component_seam()))
        base += nv
    merged = merge_mesh_component_seams(lists, native=native)
    parts = []
    for k, b in enumerate(backends):
        b.mesh_slab_link_components(merged["component_base"][k], merged["links"][k])
        parts.append(b.mesh_slab_download_components())
    out = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    out.update(n_components=merged["n_components"], lists=lists, merged=merged, counts=counts, parts=parts)
    return out


def rays_slabs_on_one_device(backends, rays, normals=False, colours=False, unit_cube=False, device="cuda:0"):
    """SlabDriver.cast_rays with ONE visible device: backends[k] owns slab k (contiguous, in z order), each with a current halo (as
    frame_slabs_on_one_device leaves it; nothing here touches a halo).  Every slab casts the same rays into its row of one gather buffer
    (tsdf_cast_rays_part_dev), backends[0] merges the rows on the device (tsdf_merge_ray_parts_dev).  Returns dict(hits, surface (None without an
    attribute), parts=[(hits, surface)] per slab, stats=[ray_stats()] per slab): hits and surface are what cast_rays of a whole-volume context gives."""
    rays = as_rays(rays)
    n, world, want_surface = len(rays), len(backends), bool(normals or colours)
    u8 = dict(dtype=torch.uint8, device=device)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 32).copy()).to(device)
    hit_parts, hits = torch.zeros((world, n, 32), **u8), torch.zeros((n, 32), **u8)
    surf_parts, surf = (torch.zeros((world, n, 32), **u8), torch.zeros((n, 32), **u8)) if want_surface else (None, None)
    torch.cuda.synchronize()                      # the contexts run on their own streams: the buffers must exist before they write them
    stats = []
    for k, b in enumerate(backends):
        b.cast_rays_part_dev(d_rays.data_ptr(), n, hit_parts[k].data_ptr(), surf_parts[k].data_ptr() if want_surface else 0, normals, colours, unit_cube)
        stats.append(b.ray_stats())               # (waits for the cast: the merge below runs on another context's stream)
    backends[0].merge_ray_parts_dev(hit_parts.data_ptr(), surf_parts.data_ptr() if want_surface else 0, world, n, n, hits.data_ptr(),
                                    surf.data_ptr() if want_surface else 0)
    backends[0].sync()
    as_hits = lambda t: t.cpu().numpy().reshape(-1).view(RAY_HIT_DTYPE)
    as_surf = lambda t: t.cpu().numpy().reshape(-1).view(RAY_SURFACE_DTYPE)
    return dict(hits=as_hits(hits), surface=as_surf(surf) if want_surface else None, stats=stats,
                parts=[(as_hits(hit_parts[k]), as_surf(surf_parts[k]) if want_surface else None) for k in range(world)])


def mesh_parts_on_one_device(backends, tag=0):
    """SlabDriver.stream_mesh with ONE visible device: backends[k] owns slab k (contiguous, in z order), each with a part ring configured
    (mesh_stream_config(part=True)) and a current halo.  Every slab queues its part, then every part is taken; nothing travels between the slabs.
    Returns (parts, frame): parts[k] = (vertices, codes, info) of slab k, frame = join_mesh_parts(parts), or None when a part overflowed.  With
    taps=True on every part ring the parts' info["taps"] are joined into the frame's info["taps"] by concatenation."""
    for b in backends:
        b.mesh_stream(tag)
    parts = [b.mesh_stream_take(wait=True) for b in backends]
    return parts, (None if any(p[2]["overflow"] for p in parts) else join_mesh_parts(parts))


def frame_slabs_on_one_device(backends, mv, proj, device, halo="exchange", composite="dense"):
    """The same partition with ONE visible device (SURVEY.md §8e fallback): the slabs run one after another and the
    "collectives" are device-to-device copies.  Used to check slab results against the unpartitioned volume on a 1-GPU box.
    backends[k] owns slab k; the composite lands in backends[0]."""
    world = len(backends)
    npx = backends[0].view[0] * backends[0].view[1]
    if halo == "exchange":
        layers, nbytes = backends[0].halo_info()
        faces = torch.empty((world, 2, nbytes // 4), dtype=torch.float32, device=device)
    for k, b in enumerate(backends):
        b.clearOccupiedBricks(); b.markBricks(); b.updateOccupiedBricks(False)
        b.integrate()
        if halo == "exchange":
            b.halo_pack_dev(faces[k, 0].data_ptr(), faces[k, 1].data_ptr())
        b.sync()
    parts = torch.zeros((world, npx * 6 if composite == "dense" else 8 + npx * 8), dtype=torch.float32, device=device)
    torch.cuda.synchronize()                      # the contexts run on their own streams: the buffers must exist before they write them
    for k, b in enumerate(backends):
        if halo == "exchange":
            below = faces[k - 1, 1].data_ptr() if k > 0 else 0
            above = faces[k + 1, 0].data_ptr() if k < world - 1 else 0
            b.halo_unpack_dev(below, above)
        b.draw(mv, proj)
        if composite == "dense":
            b.export_partial_dev(parts[k].data_ptr())
        else:
            b.export_hits_dev(parts[k].data_ptr(), npx)
        b.sync()
    if composite == "dense":
        backends[0].composite_dev(parts.data_ptr(), world)
    else:
        backends[0].composite_hits_dev(parts.data_ptr(), world, parts.stride(0) * 4)
    backends[0].fillColors()
    backends[0].sync()
