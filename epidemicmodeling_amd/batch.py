"""Batched device-resident execution of the EKF/EKS hot path.

PyTorch is used here only as plumbing -- device memory (torch tensors), the current HIP stream and,
for N > 1 GPUs, torch.distributed over RCCL.  All arithmetic happens in libepiekf.so's HIP kernels,
reached through the C ABI of include/epiekf.h with raw device pointers."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _call, _lib
from . import layout as L
from ._call import _rtwin_names, check_lasso_folds, lasso_folds  # noqa: F401  (their home is _call; public here)

OUT_NAMES = ["u_opt", "u_opt_smooth", "S_MINUS", "S_PLUS", "S_SMOOTH", "P_MINUS", "P_PLUS", "P_SMOOTH",
             "K_GAIN", "innovations", "rho"]


def out_mask_of(names) -> int:
    m = 0
    for n in names:
        m |= L.OUT_BITS[n]
    return m


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class DeviceBackend:
    """The device entry points' side of a family call (_call): inputs become contiguous tensors on `device`, outputs are
    allocated there, the call is enqueued on `stream` (default: the device's current stream)."""
    kind, checks_folds = "run_device", True
    _DTYPES = {np.float64: torch.float64, np.int32: torch.int32, np.float32: torch.float32}

    def __init__(self, device, stream=None):
        self.device, self.stream, self.keep = torch.device(device), stream, []

    def _put(self, v, dtype):
        if v is not None:
            v = v.to(self.device, dtype).contiguous()
            self.keep.append(v)
        return v

    def f64(self, v):
        return self._put(v if v is None or isinstance(v, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64),
                         torch.float64)

    def i32(self, v):
        return self._put(v if v is None or isinstance(v, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32)),
                         torch.int32)

    def f32(self, v):
        return self._put(v if v is None or isinstance(v, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(v, dtype=np.float32)),
                         torch.float32)

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=self._DTYPES[dtype], device=self.device)

    ptr = staticmethod(_ptr)

    def resident(self, v):
        return isinstance(v, torch.Tensor)

    def host(self, v):
        return v.cpu().numpy() if isinstance(v, torch.Tensor) else v

    def tail(self):
        st = torch.cuda.current_stream(self.device) if self.stream is None else self.stream
        return C.c_void_p(st.cuda_stream)


class DeviceWorkload:
    """Inputs of one batched filter problem resident in HBM (built once, run many times)."""

    def __init__(self, w, device="cuda:0"):
        self.device = torch.device(device)
        self.model, self.T, self.n_npi, self.L, self.order, self.obs_type = w.model, w.T, w.n_npi, w.L, w.order, w.obs_type
        self.m = L.MODEL_DIM[w.model]
        self.B, self.Sx, self.Su = w.B, w.Sx, w.Su
        f = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(self.device)
        i = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(self.device)
        self.x, self.u, self.R_series, self.R_scalar = f(w.x), f(w.u), f(w.R_series), f(w.R_scalar)
        self.x_series, self.u_series = i(w.x_series), i(w.u_series)
        self.prm, self.s_init, self.Ps_init = f(w.prm), f(w.s_init), f(w.Ps_init)
        self.s_final, self.Ps_final, self.Q = f(w.s_final), f(w.Ps_final), f(w.Q)
        self.r_mode = 1 if w.R_series is not None else 0
        self.q_mode = 1 if np.ndim(w.Q) == 3 else 0     # Q [T][m*m][B]: Q(:,:,k) per filter step

    def inputs_struct(self):
        s = _lib.Inputs()
        for n in ("x_series", "u_series", "x", "u", "R_series", "R_scalar", "prm", "s_init", "Ps_init",
                  "s_final", "Ps_final", "Q"):
            setattr(s, n, _ptr(getattr(self, n)))
        return s

    def input_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.x, self.u, self.R_series, self.R_scalar, self.prm,
                                                          self.s_init, self.Ps_init, self.s_final, self.Ps_final,
                                                          self.Q, self.x_series, self.u_series) if t is not None)


class EkfRunner:
    """Pre-allocated outputs + workspace for a DeviceWorkload; run() only enqueues kernels."""

    def __init__(self, dw: DeviceWorkload, outputs=None, extras=False, time_pipe=0, precheck=True, lane_block=0, shape=0,
                 storage="f64", exact_nonfinite=None, slab=None, test_window=0, test_flags=0):
        """time_pipe: epi_batch_desc.time_pipe (0 = the library decides whether a full call runs its forward kernel in time
        segments with the pinv grid of each segment beside the next, 1 = on, -1 = off).  precheck: ask the
        library once (synchronously) whether the batch qualifies for the symmetric-packed kernels, so that
        run() enqueues only the variant that will actually execute.  lane_block: 0 = classic [T][rows][B] outputs;
        8 / "auto" (= chains per wavefront of the launch) = chain-blocked outputs (epi_batch_desc.lane_block): `out` then holds the raw blocked tensors
        [T, nblk, rows, blk] ([T, nblk*blk] for one-row arrays) and unblocked() returns [T, rows, B] copies."""
        self.dw = dw
        names = list(OUT_NAMES) if outputs is None else list(outputs)
        if dw.model.startswith("NewCase") and "u_opt_smooth" in names:
            names.remove("u_opt_smooth")          # the reference has no such output (NewCase...m:1)
        self.names = names
        self.mask = out_mask_of(names)
        self.desc = _lib.make_desc(dw.model, dw.B, dw.T, dw.Sx, dw.Su, dw.n_npi, dw.L, dw.order, dw.obs_type,
                                   dw.r_mode, self.mask, dw.q_mode)
        # epi_batch_desc.shape: 0 = by batch size, 1 / 2 = one / four lanes per chain (6-state generic models)
        self.desc.shape = {"auto": 0, "lane": 1, "quad": 2, "wave": 3, "hex": 4}.get(shape, shape)
        # epi_batch_desc.storage: "f32" = outputs stored as float32 (each the fp64 result rounded once; BASELINE config 5)
        self.desc.storage = {"f64": 0, "f32": 1}[storage]
        # epi_batch_desc.exact_nonfinite: chains whose covariance overflows are run again by the dense kernels, in place
        # (their Inf / NaN pattern is then the dense evaluation's, i.e. the reference's)
        # None = the library's default (on whenever the smoother runs), True = always, False = off
        self.desc.exact_nonfinite = 0 if exact_nonfinite is None else (1 if exact_nonfinite else -1)
        # test hooks (epi_batch_desc.test_window / test_flags, 0 in production): short addressing windows, forced reverse-time pipeline
        self.desc.test_window, self.desc.test_flags = int(test_window), int(test_flags)
        odt = torch.float32 if storage == "f32" else torch.float64
        if lane_block == "auto":       # one block per wavefront of the launch
            lane_block = int(_lib.lib().epi_ekf_preferred_lane_block(C.byref(self.desc)))
        self.blk = dw.B if (lane_block <= 0 or lane_block >= dw.B) else int(lane_block)
        self.nblk = (dw.B + self.blk - 1) // self.blk
        self.desc.lane_block = 0 if self.blk == dw.B else self.blk
        self.err = C.create_string_buffer(256)
        h = _lib.lib()
        _lib.check(h.epi_ekf_validate(C.byref(self.desc), self.err), self.err)
        dev = dw.device
        self.out = {}
        shapes = {}
        for n in names:
            rows = L.out_rows(n, dw.m, dw.n_npi)
            if self.blk == dw.B:
                shapes[n] = (dw.T, dw.B) if rows == 0 else (dw.T, rows, dw.B)
            else:
                shapes[n] = (dw.T, self.nblk * self.blk) if rows == 0 else (dw.T, self.nblk, rows, self.blk)
        self.ws_bytes = int(h.epi_ekf_workspace_bytes(C.byref(self.desc)))
        self._shapes, self._odt, self._slab_opt = shapes, odt, slab
        self._allocate()
        self.pinv_rank = torch.empty((dw.T, self.nblk * self.blk), dtype=torch.int32, device=dev) if extras else None
        self.status = torch.zeros((dw.B,), dtype=torch.int32, device=dev) if extras else None
        self.ins = dw.inputs_struct()
        self.desc.time_pipe = int(time_pipe)
        self._sweep = None
        if precheck:
            ok = C.c_int(0)
            st = torch.cuda.current_stream(dev)
            rc = h.epi_ekf_precheck_device(C.byref(self.desc), C.byref(self.ins), C.c_void_p(st.cuda_stream),
                                           C.byref(ok), self.err)
            _lib.check(rc, self.err)
            self.desc.path_hint = 1 if ok.value else 2
        self._bind()

    def _allocate(self):
        """The outputs and the workspace (fresh device memory; `out` / `ws` are replaced)."""
        dw, names, shapes, odt, slab = self.dw, self.names, self._shapes, self._odt, self._slab_opt
        dev = dw.device
        self.out = {}
        ws_elems = (max(self.ws_bytes, 8) + 7) // 8
        if slab is None:
            for n in names:
                self.out[n] = torch.empty(shapes[n], dtype=odt, device=dev)
            self.ws = torch.empty(ws_elems, dtype=torch.float64, device=dev)
            self._slab = None
        else:
            # ONE device allocation for every output and the workspace (slab = {"align": bytes, "stagger": bytes}): array i
            # starts at a multiple of `align` plus i * `stagger` -- the arrays' relative placement is then the caller's choice
            # instead of the allocator's (profiles/alloc_probe.py)
            align, stagger = int(slab.get("align", 2 << 20)), int(slab.get("stagger", 0))
            isz = torch.empty((), dtype=odt).element_size()
            offs, off = {}, 0
            for i, n in enumerate(names + ["__ws__"]):
                nbytes = ws_elems * 8 if n == "__ws__" else int(np.prod(shapes[n])) * isz
                off = (off + align - 1) // align * align + i * stagger
                offs[n] = (off, nbytes)
                off += nbytes
            self._slab = torch.empty(off, dtype=torch.uint8, device=dev)
            for n in names:
                o, nb = offs[n]
                self.out[n] = self._slab[o:o + nb].view(odt).view(shapes[n])
            o, nb = offs["__ws__"]
            self.ws = self._slab[o:o + nb].view(torch.float64)

    def _bind(self):
        self.outs = _lib.Outputs()
        for n in OUT_NAMES:
            setattr(self.outs, n, _ptr(self.out.get(n)))
        self.outs.pinv_rank = _ptr(self.pinv_rank)
        self.outs.status = _ptr(self.status)

    def stage_ms(self, passes=2, min_ms=0.0, stream=None):
        """(forward, pinv, smoother) milliseconds of a pass enqueued stage by stage -- epi_ekf_time_stages_device: HIP events on
        the stream, one untimed round, then the mean over as many rounds as fill `min_ms` of device time (at least `passes`)."""
        st = torch.cuda.current_stream(self.dw.device) if stream is None else stream
        ms = (C.c_double * 3)()
        best = None
        # the library times until min_ms is filled; `passes` rounds at least: ask again while fewer were averaged
        need = float(min_ms)
        for _ in range(max(1, int(passes))):
            rc = _lib.lib().epi_ekf_time_stages_device(C.byref(self.desc), C.byref(self.ins), C.byref(self.outs), _ptr(self.ws),
                                                       self.ws_bytes, C.c_void_p(st.cuda_stream), need, ms, self.err)
            _lib.check(rc, self.err)
            cur = (float(ms[0]), float(ms[1]), float(ms[2]))
            best = cur if best is None else tuple((a + b) for a, b in zip(best, cur))
            if need > 0:
                return cur
        return tuple(x / max(1, int(passes)) for x in best)

    def tune_placement(self, tries=3, spinup_ms=150.0):
        """Where the allocator puts the ~14 arrays a pass streams concurrently changes the forward kernel's and the smoother's
        time by up to 15 % (they meet in the physically indexed L2's sets and banks or they do not: DESIGN.md 5, "where the
        arrays lie"), it is a property of the ALLOCATION -- the same arrays give the same time run after run -- and the caller
        cannot see it.  So: time a staged pass on this allocation, allocate the outputs and the workspace again (`tries` - 1
        times, each while the earlier ones are still held, so that other memory is handed out), keep the fastest and free the
        rest.  One-time set-up cost: a few passes and, transiently, `tries` x the outputs' memory (skipped when that does not
        fit).  The device is brought to its steady clocks first (`spinup_ms` of passes: after idle the first 50-150 ms of work
        run up to 15 % slower, which would make the FIRST try look bad whatever its placement) and every try is timed over at
        least 15 ms of work.  Returns {"tries": [...ms per try...], "chosen": i}.
        Call it BEFORE anything keeps a reference to `out` / `ws`: when another allocation than the first is kept (`generation`
        is then incremented), tensors taken from `out` earlier and HIP graphs captured from earlier run() calls still point at
        memory this runner no longer writes.  A later allocation is kept only if it wins by more than 1 %."""
        import time
        dev = self.dw.device
        if int(tries) > 1 and spinup_ms > 0:
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < spinup_ms:      # stage by stage, like the timed tries: one kind of launch per kernel
                self.run(phase=1); self.run(phase=3); self.run(phase=4)
                torch.cuda.synchronize(dev)
        held, log = [], []
        need = sum(t.numel() * t.element_size() for t in self.out.values()) + self.ws.numel() * 8
        for i in range(max(1, int(tries))):
            if i > 0:
                free, _ = torch.cuda.mem_get_info(dev)
                if free < need * 1.05:
                    break
                self._allocate()
                self._bind()
            f, p, b = self.stage_ms(min_ms=15.0)
            log.append({"fwd_ms": f, "pinv_ms": p, "bwd_ms": b, "sum_ms": f + p + b})
            held.append((self.out, self.ws, self._slab))
        best = int(np.argmin([x["sum_ms"] for x in log]))
        if best != 0 and log[best]["sum_ms"] > 0.99 * log[0]["sum_ms"]:
            best = 0                      # inside the timing noise: the first allocation stays
        self.generation = getattr(self, "generation", 0) + (1 if best != 0 else 0)
        self.out, self.ws, self._slab = held[best]
        self._bind()
        del held
        torch.cuda.empty_cache()
        return {"tries": log, "chosen": best}

    def run(self, stream=None, phase: int = 0):
        """Enqueue forward + backward kernels on `stream` (default: torch's current stream).
        phase 1 / 2 enqueue only the forward / only the smoother kernel (per-kernel timing)."""
        st = torch.cuda.current_stream(self.dw.device) if stream is None else stream
        self.desc.phase = phase
        rc = _lib.lib().epi_ekf_run_device(C.byref(self.desc), C.byref(self.ins), C.byref(self.outs),
                                           _ptr(self.ws), self.ws_bytes, C.c_void_p(st.cuda_stream), self.err)
        _lib.check(rc, self.err)
        return self.out

    def run_sweep(self, t_hist, sp, J0_prefix, J1_prefix, n_regions=None, stream=None):
        """epi_sweep_run_device: the full filter call followed by the sweep's scoring tail (TrainPredictPrescribeNPI.m:
        481-493) on the last T - t_hist days of the u_opt_smooth it wrote and, when `n_regions` is given (the batch then
        holds n_regions x P chains, region-major), the Pareto filter and optimum per region (:624-633) -- one library
        call, scoring and filter enqueued beside the smoother's pass over the observed days.  sp [48, B], J0_prefix /
        J1_prefix [B] as for score_sweep.  Returns dict J0, J1 [B] (views of JJ [2, B]) (+ on_front bool-able int32 [R, P],
        i_opt int32 [R])."""
        dev = self.dw.device
        B = self.dw.B
        if self._sweep is None:
            jj = torch.empty((2, B), dtype=torch.float64, device=dev)     # (J0; J1) side by side: what the end-of-sweep gather sends
            self._sweep = {"JJ": jj, "J0": jj[0], "J1": jj[1]}
        res = self._sweep
        sd = _lib.SweepDesc()
        sd.abi_version, sd.t_hist = _lib.ABI_VERSION, int(t_hist)
        if n_regions:
            P = B // int(n_regions)
            if P * int(n_regions) != B:
                raise ValueError("the batch does not hold the same number of cost weights for every region")
            sd.R, sd.P = int(n_regions), P
            if "on_front" not in res or tuple(res["on_front"].shape) != (int(n_regions), P):
                res["on_front"] = torch.empty((int(n_regions), P), dtype=torch.int32, device=dev)
                res["i_opt"] = torch.empty((int(n_regions),), dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev) if stream is None else stream
        self.desc.phase = 0
        rc = _lib.lib().epi_sweep_run_device(C.byref(self.desc), C.byref(self.ins), C.byref(self.outs), _ptr(self.ws), self.ws_bytes,
                                             C.byref(sd), _ptr(sp), _ptr(J0_prefix), _ptr(J1_prefix), _ptr(res["J0"]), _ptr(res["J1"]),
                                             _ptr(res.get("on_front")) if n_regions else None,
                                             _ptr(res.get("i_opt")) if n_regions else None, C.c_void_p(st.cuda_stream), self.err)
        _lib.check(rc, self.err)
        return res

    def unblocked(self, name):
        """[T, rows, B] ([T, B]) tensor of output `name` whatever the layout run() wrote it in."""
        t = self.pinv_rank if name == "pinv_rank" else self.out[name]
        if self.blk == self.dw.B:
            return t
        if t.dim() == 2:
            return t[:, :self.dw.B]
        T, nb, rows, blk = t.shape
        return t.permute(0, 2, 1, 3).reshape(T, rows, nb * blk)[:, :, :self.dw.B]

    def unblocked_at(self, name, t):
        """[rows, B] slice of output `name` at time index t (no copy of the whole array)."""
        x = self.out[name][t]
        if self.blk == self.dw.B:
            return x
        if x.dim() == 1:
            return x[:self.dw.B]
        nb, rows, blk = x.shape
        return x.permute(1, 0, 2).reshape(rows, nb * blk)[:, :self.dw.B]

    def output_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.out.values())


def run_workload(w, outputs=None, device="cuda:0", extras=True, time_pipe=0, precheck=True, lane_block=0, shape=0, storage="f64",
                 exact_nonfinite=None, test_window=0, test_flags=0):
    """Convenience: upload `w`, run once, return dict name -> numpy array [T, rows, B] (+ pinv_rank/status)."""
    dw = DeviceWorkload(w, device)
    r = EkfRunner(dw, outputs, extras=extras, time_pipe=time_pipe, precheck=precheck, lane_block=lane_block, shape=shape, storage=storage,
                  exact_nonfinite=exact_nonfinite, test_window=test_window, test_flags=test_flags)
    r.run()
    torch.cuda.synchronize(dw.device)
    res = {n: r.unblocked(n).cpu().numpy() for n in r.out}
    if extras:
        res["pinv_rank"] = r.unblocked("pinv_rank").cpu().numpy()
        res["status"] = r.status.cpu().numpy()
    return res


def shard_chains(B: int, rank: int, world: int):
    """Contiguous block partition of the chain axis: chains are independent, so a rank
    only ever needs its own block; returns (start, stop)."""
    per = (B + world - 1) // world
    lo = min(B, rank * per)
    return lo, min(B, lo + per)


def gather_to_root(t: torch.Tensor, group=None, dst: int = 0):
    """The path's only collective: gather per-rank result shards (chain-minor tensors of equal shape)
    to rank `dst` at the end of a sweep.  Over RCCL this is one send per peer on its own xGMI link.  The collective is
    issued whatever the world size (a one-rank world runs it too: same code path as N ranks)."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    if dist.get_backend(group) != "nccl":
        t = t.cpu()                     # gloo rehearsal / CPU tests: the gather goes through host memory
    bufs = [torch.empty_like(t) for _ in range(world)] if dist.get_rank(group) == dst else None
    dist.gather(t, bufs, dst=dst, group=group)      # RCCL: one send per peer, each on its own xGMI link
    return bufs


def blocks_side_by_side(buf: torch.Tensor) -> torch.Tensor:
    """[world, ..., per] (what all_gather_into_tensor fills: one padded block per rank) -> [..., world * per], the blocks
    next to each other in rank (= chain) order."""
    world, per = buf.shape[0], buf.shape[-1]
    return buf.movedim(0, -2).reshape(tuple(buf.shape[1:-1]) + (world * per,))


_GATHER_BUFS = {}       # (device, dtype, shape of a padded block, world) -> (send block, receive buffer): allocated once per sweep shape


def gather_shards_to_root(t: torch.Tensor, B_total: int, group=None, dst: int = 0):
    """Strong-scaling form of the end-of-sweep gather: `t` [..., n_r] holds this rank's block of a chain-minor result whose
    blocks come from shard_chains(B_total, rank, world) -- all of length ceil(B_total / world) except a shorter (possibly
    empty) last one.  Blocks are padded to the common length, gathered to rank `dst` (one message per peer) and
    reassembled there in chain order; returns the [..., B_total] tensor on `dst`, None elsewhere.  The padded send block and
    the receive buffer are allocated on the first call for a shape and reused: a pass costs one copy into the send block
    (only when the block is short or not contiguous) and the collective, no allocation."""
    import torch.distributed as dist
    world = dist.get_world_size(group)
    per = (B_total + world - 1) // world
    nccl = dist.get_backend(group) == "nccl"
    if t.shape[-1] == per and t.is_contiguous():
        send = t
        key = (t.device, t.dtype, tuple(t.shape), world)
        if nccl and key not in _GATHER_BUFS:
            _GATHER_BUFS[key] = (None, torch.empty((world,) + tuple(t.shape), dtype=t.dtype, device=t.device))
    else:
        shape = tuple(t.shape[:-1]) + (per,)
        key = (t.device, t.dtype, shape, world)
        if key not in _GATHER_BUFS or _GATHER_BUFS[key][0] is None:
            _GATHER_BUFS[key] = (torch.zeros(shape, dtype=t.dtype, device=t.device),
                                 torch.empty((world,) + shape, dtype=t.dtype, device=t.device) if nccl else None)
        send = _GATHER_BUFS[key][0]
        send[..., :t.shape[-1]].copy_(t)          # the padding stays zero
    if nccl:
        # RCCL: one ncclAllGather of the small per-chain summaries (16 B per chain) -- every rank receives
        # them, rank `dst` uses them.  Issued for every world size, one rank included.
        buf = _GATHER_BUFS[key][1]
        dist.all_gather_into_tensor(buf, send, group=group)
        if dist.get_rank(group) != dst:
            return None
        return blocks_side_by_side(buf)[..., :B_total]
    parts = gather_to_root(send, group=group, dst=dst)
    if dist.get_rank(group) != dst:
        return None
    return torch.cat([p_.to(t.device) for p_ in parts], dim=-1)[..., :B_total]


# ---------------------------------------------------------------------------
# forward simulators (Tools/SIalpha_Controlled.m, Tools/SEIRP.m, Tools/NPICost.m) on the device
# ---------------------------------------------------------------------------
SIM_FIELDS = {"s0": 0, "i0": 1, "alpha0": 2, "alpha_min": 3, "alpha_max": 4, "gamma": 5, "b": 6, "beta": 7,
              "s_noise_std": 8, "i_noise_std": 9, "alpha_noise_std": 10, "dt": 11}
SIM_A, SIM_U_MAX, SIM_W, SIM_PRM_COUNT = 12, 24, 36, 48


def normal_draws(nt, rows, lanes, seed, stream=0, t0=0, lane0=0, dtype=torch.float64, device="cuda:0", cuda_stream=None):
    """Standard-normal draws from a seed, generated on the device (epi_noise_fill_device): the window
    [t0, t0 + nt) x rows x [lane0, lane0 + lanes) of the logical array of (seed, stream) as a device tensor [nt, rows, lanes],
    float64 or float32 (the float64 draw rounded once).  rows is 1 or 3, seed a 64-bit integer, stream < 2^30.  The value of
    draw (t, row, lane) is a pure function of (seed, stream, t, row, lane): Philox4x32-10, then the inverse normal CDF (AS241),
    |z| <= 8.2096.  A call with seed= / noise_stream= equals, bit for bit, the same call given z = normal_draws(...) of its z's
    shape (`stream` here is the noise stream, as in the descriptor; the HIP stream is `cuda_stream`).
    Enqueued on `cuda_stream` (default: the current stream) without a host synchronisation."""
    if dtype not in (torch.float64, torch.float32):
        raise ValueError("dtype must be torch.float64 or torch.float32")
    dev = torch.device(device)
    st = torch.cuda.current_stream(dev) if cuda_stream is None else cuda_stream
    with torch.cuda.stream(st):
        return _call.normal_draws(DeviceBackend(dev, st), nt, rows, lanes, seed, stream, t0, lane0, dtype == torch.float32)


def sialpha_sim(u, sp, z=None, u_series=None, with_cost=False, store=True, device="cuda:0", seed=None, noise_stream=0):
    """Batched SIalpha_Controlled (+ fused NPICost).  u [K, n_npi, Su], sp [48, B] (SIM_* rows), z [K, 3, B]
    standard-normal draws or None; or seed= (and noise_stream=): the draws normal_draws(K, 3, B, seed, noise_stream) generated inside the
    kernel (seed and z together raise).  Returns dict of torch tensors s,i,alpha [K,B] (+ J0,J1 [B])."""
    noise = _lib.noise_of(seed, noise_stream, z)
    dev = torch.device(device)
    t = lambda a, dt=torch.float64: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev) \
        if not isinstance(a, torch.Tensor) else a
    u, sp, z = t(u), t(sp), t(z)
    us = t(u_series, torch.int32)
    K, n_npi, Su = u.shape
    B = sp.shape[1]
    d = _lib.SimDesc()
    d.abi_version, d.B, d.K, d.Su, d.n_npi = _lib.ABI_VERSION, B, K, Su, n_npi
    d.noise, d.with_cost, d.prefix_days = int(z is not None), int(with_cost), 0
    out = {}
    if store:
        for n in ("s", "i", "alpha"):
            out[n] = torch.empty((K, B), dtype=torch.float64, device=dev)
    if with_cost:
        out["J0"] = torch.empty((B,), dtype=torch.float64, device=dev)
        out["J1"] = torch.empty((B,), dtype=torch.float64, device=dev)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream(dev)
    tail = (_ptr(us), _ptr(u), _ptr(sp), _ptr(z), _ptr(out.get("s")), _ptr(out.get("i")), _ptr(out.get("alpha")), _ptr(out.get("J0")),
            _ptr(out.get("J1")), C.c_void_p(st.cuda_stream), err)
    if noise is None:
        rc = _lib.lib().epi_sialpha_sim_device(C.byref(d), *tail)
    else:
        rc = _lib.lib().epi_sialpha_sim_device_seeded(C.byref(d), C.byref(noise), *tail)
    _lib.check(rc, err)
    return out


def random_npi_mc(sp, u_min, n_scen, K, seed=0, z=None, J0_prefix=None, J1_prefix=None, prefix_days=0,
                  store_u=False, device="cuda:0", noise_seed=None, noise_stream=0):
    """Random-NPI Monte-Carlo scenarios (Tools/TrainPredictPrescribeNPI.m:496-521) on the device.

    sp [48, R] per-region SIM_* rows (end-of-history state, model constants, SIM_U_MAX = NPI_MAXES, SIM_W = NPICost
    weights), u_min [n_npi, R] = NPI_MINS, z [K, 3, n_scen*R] standard-normal draws or None; J0_prefix/J1_prefix [R]
    sequential historic sums over prefix_days.  `seed` keys the integer draws of the plans, as ever; noise_seed= (and noise_stream=)
    asks for the state noise normal_draws(K, 3, n_scen*R, noise_seed, noise_stream) generated inside the kernel (noise_seed and z
    together raise).  The two may be the same number: their Philox counters never meet.  Returns dict J0, J1 [n_scen, R]
    (+ u [K, n_npi, n_scen*R])."""
    noise = _lib.noise_of(noise_seed, noise_stream, z)
    dev = torch.device(device)
    t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else
                                          torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev))
    sp, u_min, z, J0p, J1p = t(sp), t(u_min), t(z), t(J0_prefix), t(J1_prefix)
    n_npi, R = u_min.shape
    d = _lib.McDesc()
    d.abi_version, d.R, d.n_scen, d.K, d.n_npi = _lib.ABI_VERSION, R, int(n_scen), int(K), n_npi
    d.noise, d.prefix_days = int(z is not None), int(prefix_days)
    d.seed_lo, d.seed_hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    out = {"J0": torch.empty((n_scen, R), dtype=torch.float64, device=dev),
           "J1": torch.empty((n_scen, R), dtype=torch.float64, device=dev)}
    if store_u:
        out["u"] = torch.empty((K, n_npi, n_scen * R), dtype=torch.float64, device=dev)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream(dev)
    tail = (_ptr(sp), _ptr(u_min), _ptr(z), _ptr(J0p), _ptr(J1p), _ptr(out.get("u")), _ptr(out["J0"]), _ptr(out["J1"]),
            C.c_void_p(st.cuda_stream), err)
    if noise is None:
        rc = _lib.lib().epi_random_npi_mc_device(C.byref(d), *tail)
    else:
        rc = _lib.lib().epi_random_npi_mc_device_seeded(C.byref(d), C.byref(noise), *tail)
    _lib.check(rc, err)
    return out


def pareto_front(J0, J1, n_regions):
    """Pareto-front filter and optimum of the sweep (Tools/TrainPredictPrescribeNPI.m:624-633) per region.
    J0, J1: torch [B] in the sweep's chain order (region-major).  Returns (on_front bool [R, P], i_opt int [R],
    0-based)."""
    dev = J0.device
    B = J0.numel()
    P = B // n_regions
    if P * n_regions != B:
        raise ValueError("J0 does not hold the same number of points for every region")
    on = torch.empty((n_regions, P), dtype=torch.int32, device=dev)
    io = torch.empty((n_regions,), dtype=torch.int32, device=dev)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream(dev)
    rc = _lib.lib().epi_pareto_front_device(n_regions, P, _ptr(J0.contiguous()), _ptr(J1.contiguous()), _ptr(on),
                                            _ptr(io), C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    return on.bool(), io


def si_controlled(alpha, beta, s0, i0, K, dt, alpha_series=None, device="cuda:0"):
    """Batched Tools/SI_Controlled.m: alpha [K-1, Sa], beta / s0 / i0 [B].  Returns (s, i) torch [K, B]."""
    dev = torch.device(device)
    t = lambda a, dt_=torch.float64: None if a is None else (a.contiguous() if isinstance(a, torch.Tensor) else
                                                             torch.as_tensor(np.ascontiguousarray(a), dtype=dt_).to(dev))
    al, ser = t(alpha), t(alpha_series, torch.int32)
    prm = t(np.stack([np.asarray(beta, dtype=np.float64), np.asarray(s0, dtype=np.float64), np.asarray(i0, dtype=np.float64)]))
    B = prm.shape[1]
    if al.shape[0] < K - 1:
        raise IndexError("Index exceeds the number of array elements (alpha).")
    s = torch.empty((K, B), dtype=torch.float64, device=dev); i = torch.empty_like(s)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream(dev)
    rc = _lib.lib().epi_si_controlled_device(B, int(K), al.shape[1], float(dt), _ptr(ser), _ptr(al), _ptr(prm), _ptr(s), _ptr(i),
                                             C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    return s, i


def npi_cost(newcases, inputs, weights, u_series=None, device="cuda:0"):
    """Batched Tools/NPICost.m: newcases [T, B], inputs [T, n_npi, Su], weights [T, n_npi, B] or [n_npi, B] (the same
    every day).  Returns (J0, J1) torch [B]."""
    dev = torch.device(device)
    t = lambda a, dt=torch.float64: None if a is None else (a.contiguous() if isinstance(a, torch.Tensor) else
                                                            torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev))
    nc, u, w, us = t(newcases), t(inputs), t(weights), t(u_series, torch.int32)
    T, B = nc.shape
    n_npi, Su = u.shape[1], u.shape[2]
    if u.shape[0] != T or w.shape[-1] != B or w.shape[-2] != n_npi or (w.dim() == 3 and w.shape[0] != T):
        raise ValueError("NPICost: newcases, inputs and weights do not agree in size")
    J0 = torch.empty((B,), dtype=torch.float64, device=dev); J1 = torch.empty_like(J0)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream(dev)
    rc = _lib.lib().epi_npi_cost_device(B, T, n_npi, Su, int(w.dim() == 3), _ptr(us), _ptr(nc), _ptr(u), _ptr(w), _ptr(J0),
                                        _ptr(J1), C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    return J0, J1


def preprocess(cases, population, deaths=None, ip=None, W=7, min_cases=1.0, first_num_days=7, outputs=None,
               device="cuda:0"):
    """Per-region preprocessing on the device (Tools/TrainPredictPrescribeNPI.m:142-198,201-202,240).

    cases / deaths: cumulative confirmed counts [T, S] (NaN = missing), population [S], ip [T, n_npi, S] (NaN = N/A).
    Returns dict of torch tensors in the filters' input layout: x_new / x_total / R_v / new_refined / new_smoothed /
    zero_lag / fatality [T, S], I0 [S], ip_filled [T, n_npi, S] (those in `outputs`; default: all that apply)."""
    dev = torch.device(device)
    t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else
                                          torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev))
    cases, population, deaths, ip = t(cases), t(population), t(deaths), t(ip)
    T, S = cases.shape
    names = list(_lib.PRE_OUT_NAMES) if outputs is None else list(outputs)
    if deaths is None and "fatality" in names:
        names.remove("fatality")
    if ip is None and "ip_filled" in names:
        names.remove("ip_filled")
    d = _lib.PreDesc()
    d.abi_version, d.S, d.T, d.n_npi = _lib.ABI_VERSION, S, T, 0 if ip is None else ip.shape[1]
    d.W, d.first_num_days, d.min_cases = int(W), int(first_num_days), float(min_cases)
    out = {}
    for n in names:
        shape = (S,) if n == "I0" else (tuple(ip.shape) if n == "ip_filled" else (T, S))
        out[n] = torch.empty(shape, dtype=torch.float64, device=dev)
    outs = _lib.PreOutputs()
    for n in _lib.PRE_OUT_NAMES:
        setattr(outs, n, _ptr(out.get(n)))
    h = _lib.lib()
    wsb = int(h.epi_preprocess_workspace_bytes(C.byref(d)))
    ws = torch.empty(max(wsb // 8, 1), dtype=torch.float64, device=dev)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream(dev)
    rc = h.epi_preprocess_device(C.byref(d), _ptr(cases), _ptr(deaths), _ptr(population), _ptr(ip), C.byref(outs),
                                 _ptr(ws), wsb, C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    return out


def nnls_affine_fit(X, y, max_iters=100, device="cuda:0"):
    """Regression between the EKF rounds on the device (Tools/TrainPredictPrescribeNPI.m:251-276, 'NONNEGATIVELS').
    X [D, n, S] = NPI_MAXES - InterventionPlans over the regression window, y [D, S] = smoothed alpha.
    Returns dict of torch tensors a [n, S], b [S], min_err [S], iters [S], flag [S]."""
    dev = torch.device(device)
    t = lambda v: v if isinstance(v, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64).to(dev)
    X, y = t(X).contiguous(), t(y).contiguous()
    D, n, S = X.shape
    d = _lib.NnlsDesc()
    d.abi_version, d.S, d.D, d.n, d.max_iters = _lib.ABI_VERSION, S, D, n, int(max_iters)
    out = {"a": torch.empty((n, S), dtype=torch.float64, device=dev), "b": torch.empty((S,), dtype=torch.float64, device=dev),
           "min_err": torch.empty((S,), dtype=torch.float64, device=dev),
           "iters": torch.empty((S,), dtype=torch.int32, device=dev), "flag": torch.empty((S,), dtype=torch.int32, device=dev)}
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream(dev)
    rc = _lib.lib().epi_nnls_affine_fit_device(C.byref(d), _ptr(X), _ptr(y), _ptr(out["a"]), _ptr(out["b"]),
                                               _ptr(out["min_err"]), _ptr(out["iters"]), _ptr(out["flag"]),
                                               C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    return out


RT_OUT_ROWS = {"S_MINUS": 2, "S_PLUS": 2, "P_MINUS": 4, "P_PLUS": 4, "K_GAIN": 2, "S_SMOOTH": 2, "P_SMOOTH": 4,
               "innovations": 0, "rho": 0}


class RtRunner:
    """Batched Tools/Rt_ExpFitEKF.m on the device: inputs of a synth.RtWorkload resident in HBM, outputs
    pre-allocated; run() only enqueues rt_expfit_fwd (+ rt_expfit_bwd when a smoothed output is selected)."""

    def __init__(self, w, device="cuda:0", outputs=None):
        self.device = dev = torch.device(device)
        f = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev)
        self.x, self.rp = f(w.x), f(w.rp)
        self.x_series = None if w.x_series is None else torch.as_tensor(np.ascontiguousarray(w.x_series), dtype=torch.int32).to(dev)
        self.T, self.B = w.T, w.B
        names = list(_lib.RT_OUT_NAMES) if outputs is None else list(outputs)
        for n in ("S_MINUS", "S_PLUS", "P_MINUS", "P_PLUS"):      # the smoother reads them back
            if n not in names:
                names.append(n)
        self.out = {n: torch.empty((w.T, w.B) if RT_OUT_ROWS[n] == 0 else (w.T, RT_OUT_ROWS[n], w.B), dtype=torch.float64,
                                   device=dev) for n in names}
        self.desc = _lib.RtDesc()
        self.desc.abi_version, self.desc.B, self.desc.T, self.desc.Sx = _lib.ABI_VERSION, w.B, w.T, w.x.shape[1]
        self.desc.L, self.desc.order = int(w.L), int(w.order)
        self.outs = _lib.RtOutputs()
        for n in _lib.RT_OUT_NAMES:
            setattr(self.outs, n, _ptr(self.out.get(n)))
        self.err = C.create_string_buffer(256)
        _lib.check(_lib.lib().epi_rt_expfit_validate(C.byref(self.desc), self.err), self.err)

    def run(self, stream=None):
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        rc = _lib.lib().epi_rt_expfit_run_device(C.byref(self.desc), _ptr(self.x_series), _ptr(self.x), _ptr(self.rp),
                                                 C.byref(self.outs), C.c_void_p(st.cuda_stream), self.err)
        _lib.check(rc, self.err)
        return self.out


def rt_expfit(w, device="cuda:0", outputs=None):
    """Convenience: upload a synth.RtWorkload, run once, return dict name -> numpy array."""
    r = RtRunner(w, device, outputs)
    r.run()
    torch.cuda.synchronize(r.device)
    return {n: t.cpu().numpy() for n, t in r.out.items()}


def seirp_sim(par, init, dt, K, sat=None, integrator="euler", device="cuda:0"):
    """Batched SEIRP / SEIRPSaturatedResource.  par [K or 1, 7, B], init [5, B], sat [6, B] or None.
    Returns torch tensor [K, 5, B] (s,e,i,r,p rows; row 0 is the initial condition, SEIRP.m:20-24)."""
    dev = torch.device(device)
    t = lambda a: None if a is None else (a.contiguous() if isinstance(a, torch.Tensor) else
                                          torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev))
    par, init, sat = t(par), t(init), t(sat)
    B = init.shape[1]
    out = torch.empty((K, 5, B), dtype=torch.float64, device=dev)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream(dev)
    rc = _lib.lib().epi_seirp_sim_device(B, K, par.shape[0], float(dt), int(sat is not None),
                                         {"euler": 0, "rk4": 1}[integrator], _ptr(par), _ptr(init), _ptr(sat),
                                         _ptr(out), C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    return out


def score_sweep(u_opt_smooth, t_hist, sp, J0_prefix, J1_prefix, store=False, B=None):
    """Scenario scoring tail of the Pareto sweep (Tools/TrainPredictPrescribeNPI.m:481-493) on the device.

    u_opt_smooth : torch [T, n_npi, B] (the smoother's output, left in HBM) or, chain-blocked, [T, nblk, n_npi, blk]
                   (then pass the number of chains B); its last T - t_hist days drive
                   SIalpha_Controlled from the end-of-history state given in `sp` (SIM_* rows, [48, B]);
    J0_prefix/J1_prefix : [B] sequential sums over the t_hist historic days (newcases; weights.*inputs).
    Returns dict with J0, J1 [B] (NPICost over the whole span) and, if store, the simulated s, i, alpha [H, B]."""
    dev = u_opt_smooth.device
    if u_opt_smooth.dim() == 4:
        T, _, n_npi, u_block = u_opt_smooth.shape
        if B is None:
            raise ValueError("blocked u_opt_smooth needs the number of chains B")
    else:
        T, n_npi, B = u_opt_smooth.shape
        u_block = 0
    H = T - t_hist
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev) if not isinstance(a, torch.Tensor) else a
    sp, J0p, J1p = t(sp), t(J0_prefix), t(J1_prefix)
    u_h = u_opt_smooth[t_hist:]                 # contiguous view: [H, n_npi, B]
    d = _lib.SimDesc()
    d.abi_version, d.B, d.K, d.Su, d.n_npi = _lib.ABI_VERSION, B, H, B, n_npi
    d.noise, d.with_cost, d.prefix_days, d.u_block = 0, 1, int(t_hist), int(u_block)
    out = {"J0": torch.empty((B,), dtype=torch.float64, device=dev), "J1": torch.empty((B,), dtype=torch.float64, device=dev)}
    if store:
        for n in ("s", "i", "alpha"):
            out[n] = torch.empty((H, B), dtype=torch.float64, device=dev)
    err = C.create_string_buffer(256)
    st = torch.cuda.current_stream(dev)
    rc = _lib.lib().epi_sialpha_score_device(C.byref(d), None, _ptr(u_h), _ptr(sp), None, _ptr(J0p), _ptr(J1p),
                                             _ptr(out.get("s")), _ptr(out.get("i")), _ptr(out.get("alpha")),
                                             _ptr(out["J0"]), _ptr(out["J1"]), C.c_void_p(st.cuda_stream), err)
    _lib.check(rc, err)
    return out


LA_TABLES = ("est_plus", "est_smooth")
LA_STATS = ("mean_plus", "median_plus", "std_plus", "mean_smooth", "median_smooth", "std_smooth")


def _lookahead_arrays(w, truth, population):
    """Per-region arrays of the study in ABI order (a synth.Workload of SIAlphaModelEKF with one chain per region)."""
    if w.model != "SIAlphaModelEKF":
        raise _lib.EpiError(-8, "the look-ahead study runs SIAlphaModelEKF (EPI_MODEL_SIA3) only")
    if w.x_series is not None or w.u_series is not None or w.Sx != w.B or w.Su != w.B:
        raise ValueError("the look-ahead study takes one column per region (identity series)")
    return {"x": w.x, "u": w.u, "R_series": w.R_series, "R_scalar": w.R_scalar, "prm": w.prm, "s_init": w.s_init,
            "Ps_init": w.Ps_init, "s_final": w.s_final, "Ps_final": w.Ps_final, "Q": w.Q, "truth": truth, "population": population}


class LookaheadRunner:
    """The forecast look-ahead error study (Tools/ForecastQualityAssessment.m:359-393, 428-449) as one device call
    (epi_lookahead_run_device).  `w` holds the per-region inputs of SIAlphaModelEKF (one chain per region, identity series,
    e.g. pipeline.workload3); truth [LL, R] = NewCasesSmoothed_ENTIRE; population [R].  Inputs stay in HBM, outputs and
    workspace are pre-allocated; run() only enqueues.  out: est_plus / est_smooth [F, M, R], mean / median / std_{plus,smooth}
    [M, R] and, with chains=True, S_PLUS / S_SMOOTH [LL, 3, R * F] (chain c = r * F + start - 1) and status [R * F]."""

    def __init__(self, w, truth, population, F, M=60, device="cuda:0", chains=False, shape=0):
        self.device = dev = torch.device(device)
        arrs = _lookahead_arrays(w, truth, population)
        f = lambda a: None if a is None else (a.to(dev, torch.float64).contiguous() if isinstance(a, torch.Tensor) else
                                              torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev))
        self.inp = {k: f(v) for k, v in arrs.items()}
        R, LL = w.B, w.T
        self.R, self.LL, self.F, self.M = R, LL, int(F), int(M)
        self.desc = _lib.make_lookahead_desc(R, LL, F, M, w.n_npi, w.L, w.order, w.obs_type,
                                             1 if w.R_series is not None else 0, shape=shape)
        self.err = C.create_string_buffer(256)
        h = _lib.lib()
        _lib.check(h.epi_lookahead_validate(C.byref(self.desc), self.err), self.err)
        self.out = {n: torch.empty((self.F, self.M, R), dtype=torch.float64, device=dev) for n in LA_TABLES}
        self.out.update({n: torch.empty((self.M, R), dtype=torch.float64, device=dev) for n in LA_STATS})
        if chains:
            for n in ("S_PLUS", "S_SMOOTH"):
                self.out[n] = torch.empty((LL, 3, R * self.F), dtype=torch.float64, device=dev)
            self.out["status"] = torch.zeros((R * self.F,), dtype=torch.int32, device=dev)
        self.ws_bytes = int(h.epi_lookahead_workspace_bytes(C.byref(self.desc)))
        self.ws = torch.empty((max(self.ws_bytes, 8) + 7) // 8, dtype=torch.float64, device=dev)
        self.ins = _lib.LookaheadInputs()
        for n in _lib.LA_IN_NAMES:
            setattr(self.ins, n, _ptr(self.inp.get(n)))
        self.outs = _lib.LookaheadOutputs()
        for n in _lib.LA_OUT_NAMES:
            setattr(self.outs, n, _ptr(self.out.get(n)))

    def run(self, stream=None):
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        rc = _lib.lib().epi_lookahead_run_device(C.byref(self.desc), C.byref(self.ins), C.byref(self.outs), _ptr(self.ws),
                                                 self.ws_bytes, C.c_void_p(st.cuda_stream), self.err)
        _lib.check(rc, self.err)
        return self.out


def lookahead(w, truth, population, F, M=60, device="cuda:0", chains=False, shape=0):
    """Convenience: upload, run the study once, return dict name -> numpy array (see LookaheadRunner)."""
    r = LookaheadRunner(w, truth, population, F, M, device, chains, shape)
    r.run()
    torch.cuda.synchronize(r.device)
    return {n: t.cpu().numpy() for n, t in r.out.items()}


def lookahead_host(w, truth, population, F, M=60, device=0, chains=False, shape=0, placement_tries=0):
    """The same study through the host-pointer entry (epi_lookahead_run_host: NumPy arrays in and out, synchronous; what a
    MEX gateway would bind).  Returns the dict of lookahead()."""
    arrs = {k: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
            for k, v in _lookahead_arrays(w, truth, population).items()}
    R, LL, F, M = w.B, w.T, int(F), int(M)
    d = _lib.make_lookahead_desc(R, LL, F, M, w.n_npi, w.L, w.order, w.obs_type, 1 if w.R_series is not None else 0,
                                 shape=shape, placement_tries=placement_tries)
    out = {n: np.empty((F, M, R)) for n in LA_TABLES}
    out.update({n: np.empty((M, R)) for n in LA_STATS})
    if chains:
        out.update(S_PLUS=np.empty((LL, 3, R * F)), S_SMOOTH=np.empty((LL, 3, R * F)), status=np.zeros(R * F, dtype=np.int32))
    ins, outs = _lib.LookaheadInputs(), _lib.LookaheadOutputs()
    for n in _lib.LA_IN_NAMES:
        setattr(ins, n, None if arrs.get(n) is None else arrs[n].ctypes.data_as(C.c_void_p))
    for n in _lib.LA_OUT_NAMES:
        setattr(outs, n, out[n].ctypes.data_as(C.c_void_p) if n in out else None)
    err = C.create_string_buffer(256)
    rc = _lib.lib().epi_lookahead_run_host(C.byref(d), C.byref(ins), C.byref(outs), int(device), err)
    _lib.check(rc, err)
    return out


def rt_window(new_cases, wlen, time_unit=1.0, causal=1, generation_period=None, methods=("LogLinReg", "GenRatios", "NonlinLS"),
              device="cuda:0"):
    """Tools/Rt_ExpFitLogLinReg.m, Rt_ExpFitGenRatios.m and Rt_ExpFitNonlinLS.m over every column of new_cases [L, R] (days x
    regions: the new_smoothed layout of preprocess) in one device call (epi_rtwin_run_device).  `methods` is any subset of the
    three names (or the EPI_RTWIN_* bits); GenRatios needs generation_period.  Returns a dict of torch tensors [L, R]:
    llr_{Rt, A, Lambda, ExpFit}, gr_{Rt, Lambda, RtSmoothed, LambdaSmoothed}, nls_{Rt, A, Lambda, ExpFit} and the int32
    nls_status / nls_iters (status codes in _lib.RTWIN_STATUS), for the methods asked.  Enqueued on the current stream (where
    the input copy and the outputs are allocated) without a host synchronisation."""
    return _call.rt_window(DeviceBackend(device), new_cases, wlen, time_unit, causal, generation_period, methods)


def lasso_cv(X, y, K=50, folds=None, seed=0, num_lambda=100, lambda_ratio=1e-4, rel_tol=1e-4, max_iter=100000,
             device="cuda:0"):
    """REGRESSION_TYPE = 'LASSO' for every region in one device call (epi_lasso_run_device): lasso(X, y, 'CV', K) with
    MATLAB's defaults, our reading in DESIGN.md §4.5.  X [D, n, R] = NPI_MAXES - InterventionPlans over the regression window,
    y [D, R].  folds [D, R] int32 in 0 .. K-1 (default lasso_folds(D, K, R, seed)); K = 0 runs the path only.
    Returns a dict of torch tensors: lambda, intercept, df, iters [NL, R] (ascending lambda), B [NL, n, R], status [R] and,
    with K >= 2, mse, se [NL, R], idx_min_mse, idx_1se [R] (0-based), a [n, R] = B at idx_min_mse, b [R] its intercept.
    Enqueued on the current stream without a host synchronisation (a folds tensor already on the device is not checked
    here: a bad partition gives its regions status bad_folds)."""
    return _call.lasso_cv(DeviceBackend(device), X, y, K, folds, seed, num_lambda, lambda_ratio, rel_tol, max_iter)


def robust_affine_fit(X, y, robust=True, lower=0.0, upper=float("inf"), max_iter=50, outputs=None, device="cuda:0"):
    """REGRESSION_TYPE = 'NONNEGATIVELS-ELEMENT-WISE' for every region in one device call (epi_robfit_run_device): for every
    NPI k on its own fit(X(:,k), y, 'a*x+b', 'Robust','on', 'Lower',[lower -inf]) as bisquare iteratively reweighted least
    squares (our reading: DESIGN.md §4.10), then b = mean(y - X a).  X [D, n, R] = NPI_MAXES - InterventionPlans over the
    regression window, y [D, R].  robust=False stops after the bounded least-squares start.
    outputs: names out of a, b_item, sigma, iters, status [n, R], weights [D, n, R], b [R] (default: all but weights).
    Returns a dict of torch tensors (iters, status int32; status is a set of _lib.ROBFIT_STATUS_BITS).  Enqueued on the
    current stream without a host synchronisation."""
    return _call.robust_affine_fit(DeviceBackend(device), X, y, robust, lower, upper, max_iter, outputs)


def rate_map(ip, new_smoothed, n_train, y=None, extra=None, lambda_in=None, lags=(3, 5, 7), ridge=1e-6, lambda_threshold=0.1,
             reduction_effect=0.01, effect_lag=3, outputs=None, device="cuda:0"):
    """The NPI-to-growth-rate predictor of testScripts/test04FullFeatureExtMLpipeline.m (:292-404, :418-431, :576-642) for
    every region and every train end in one device call (epi_ratemap_run_device): the growth rate y [T, R]
    (NaN / Inf filled forward) regressed on [ip, ip lagged by each of `lags`, extra] (ip [T, n, R] N/A-filled, extra
    [T, E, R] caller-made columns), every column divided by its max(abs) over all T days, over the days 1 .. n_train[k] with
    (X'X + ridge I) m = X'y; lambda_hat = [y(1:n_train); X m] clipped to +-lambda_threshold on the test days;
    new_cases_est = [new_smoothed(1:n_train); new_smoothed(n_train) exp(cumsum(lambda_hat test days))]; tracker: the
    policy-variation increments per region.  With lambda_in [K, T, R] instead of y nothing is fitted: lambda_in is
    lambda_hat (LASSO's or the AR model's prediction) and goes through the same clip and rebuild.
    n_train: a list of K train ends (MATLAB's numTimeStepsTrain, 1 .. T), read on the host.
    outputs: names out of map [K, F, R], x_mx [F, R], y_filled [T, R], lambda_hat, new_cases_est [K, T, R], tracker [T, R],
    status [K, R] (int32, a set of _lib.RATEMAP_STATUS_BITS; default: all that apply).  Returns a dict of torch tensors.
    Enqueued on the current stream without a host synchronisation."""
    return _call.rate_map(DeviceBackend(device), ip, new_smoothed, n_train, y, extra, lambda_in, lags, ridge, lambda_threshold,
                          reduction_effect, effect_lag, outputs)


def mldivide(X, y, n_rows=None, tol_scale=1.0, outputs=None, device="cuda:0"):
    """MATLAB's rectangular backslash m = X(1:n_rows, :) \\ y(1:n_rows) of test01FitExponential.m:159, test03 :169 and test05
    :185 for every region and every row count in one device call (epi_mldiv_run_device): Householder QR
    with column pivoting on X [D, F, R] itself (F <= 96, max(n_rows) (F + 1) <= 20000), the rank by
    |R(j,j)| > tol_scale max(n_rows, F) eps |R(1,1)| (tol_scale = 1 is the rule of MATLAB's lscov.m), the basic solution;
    fitted = X m over all D rows, so the rows beyond n_rows are the prediction.  y [D, R].
    n_rows: a list of K row counts 1 .. D, read on the host (default: [D]).
    outputs: names out of m [K, F, R], rank [K, R], perm [K, F, R] (0-based, pivot order), rdiag [K, F, R], resid [K, R],
    fitted [K, D, R], status [K, R] (int32, a set of _lib.MLDIV_STATUS_BITS; default: all).  Returns a dict of torch tensors.
    Enqueued on the current stream without a host synchronisation."""
    return _call.mldivide(DeviceBackend(device), X, y, n_rows, tol_scale, outputs)


def svr(X, y, n_rows=None, kernel="linear", box=None, epsilon=None, kernel_scale=None, tol=1e-3, max_iter=100000, outputs=None,
        device="cuda:0"):
    """The fitrsvm rows of the reference's predictor block (test05DirectNewCasesLearning.m:198-268, test04 :435-445, test03
    :242-262): epsilon-insensitive support-vector regression on X(1:n_rows, :), y(1:n_rows) for every region and every row
    count in one device call (epi_svr_run_device).  X [D, F, R] (F <= 96, n_rows <= 1024,
    max(n_rows) ((F | 1) + 1) <= 20000), y [D, R].  kernel: "linear" or "gaussian" (exp(-|a - b|^2 / kernel_scale^2)).
    LIBSVM's sequential minimal optimisation from alpha = 0 until m(alpha) - M(alpha) < tol or max_iter pair steps.
    n_rows: a list of K row counts 1 .. D, read on the host (default: [D]).
    box, epsilon, kernel_scale: scalars or arrays [R] (NumPy or torch); None takes _lib.svr_defaults of y(1:max(n_rows)), which
    copies y to the host -- pass arrays to stay asynchronous.
    outputs: names out of beta [K, D, R], bias [K, R], w [K, F, R] (linear kernel only), fitted [K, D, R] (over all D rows: the
    rows beyond n_rows are the prediction), n_iter, gap, n_sv, status [K, R] (status: a set of _lib.SVR_STATUS_BITS; default:
    all).  Returns a dict of torch tensors.  Enqueued on the current stream without a host synchronisation."""
    return _call.svr(DeviceBackend(device), X, y, n_rows, kernel, box, epsilon, kernel_scale, tol, max_iter, outputs)


def ensemble_summary(src, R, D, q=_lib.ENS_DEFAULT_Q, population=None, outputs=None, stream=None):
    """Monte-Carlo ensemble statistics in one device call (epi_ens_run_device): src [T, rows, B] or [T, B]
    (float32 or float64, on the device) is an output array of B = R * D chains in the classic layout, region-major (chain =
    r * D + d: synth.make_cfg5); every (day, row, region) is summarised over its D draws.  NaN members are excluded.
    population [R] appends the derived row ((N * row0) * row1) * row2 (the day's new cases of the 3-state model).
    outputs: names out of mean, std, min, max, quantiles (default: all); count is always returned.
    Returns a dict of device tensors: mean, std, min, max [T, rows', R] float64, quantiles [T, n_q, rows', R] (MATLAB's
    quantile rule = NumPy's method="hazen"), count [T, rows', R] int32.  Enqueued on `stream` (default: the current stream)
    without a host synchronisation.  A chain-blocked output (EkfRunner(lane_block=...)) is not accepted."""
    if not isinstance(src, torch.Tensor):
        raise TypeError("src must be a torch tensor (NumPy arrays: hostapi.ensemble_summary)")
    if src.dim() == 4:
        raise ValueError("src is a chain-blocked tensor [T, nblk, rows, blk]; ensemble_summary takes the classic layout "
                         "[T, rows, B]: pass EkfRunner.unblocked(name).contiguous(), or run with lane_block=0")
    if src.dim() not in (2, 3):
        raise ValueError("src must be [T, rows, B] or [T, B]")
    if src.dtype not in (torch.float32, torch.float64):
        raise TypeError("src must be float32 or float64")
    R, D = int(R), int(D)
    if src.shape[-1] != R * D:
        raise ValueError(f"src holds {src.shape[-1]} chains, R * D = {R * D}")
    dev = src.device
    src = src.contiguous()
    T, rows = src.shape[0], (1 if src.dim() == 2 else src.shape[1])
    pop = None
    if population is not None:
        pop = (population if isinstance(population, torch.Tensor) else
               torch.as_tensor(np.ascontiguousarray(population, dtype=np.float64))).to(dev, torch.float64).contiguous()
        if tuple(pop.shape) != (R,):
            raise ValueError("population must be [R]")
    d = _lib.make_ens_desc(T, rows, R, D, q, storage=1 if src.dtype == torch.float32 else 0, derive_newcases=int(pop is not None))
    names = [k for k in _lib.ENS_OUT_NAMES if k != "count"] if outputs is None else list(outputs)
    bad = [k for k in names if k not in _lib.ENS_OUT_NAMES]
    if bad:
        raise ValueError(f"unknown outputs {bad}")
    shapes = _lib.ens_shapes(T, rows, R, d.n_q, d.derive_newcases)
    out = _call.run_family("ens", DeviceBackend(dev, stream), d, [_ptr(src), _ptr(pop)], shapes, names + ["count"])
    if src.dim() == 2:
        out = {k: v.squeeze(-2) for k, v in out.items()}
    return out


def ar_forecast(seg, beta, s0, i0, dt, p, H, D, z=None, drive=None, drive_series=None, A=None, noise_var=None, nv_mode=0,
                stream=None, device="cuda:0", seed=None, noise_stream=0):
    """The autoregressive alpha forecaster of Tools/PrescribeNPI.m:204-215 for R regions x D draws in one device call
    (epi_arfc_run_device): ar(seg, p) -> filtic -> filter(sqrt(nv), A, z, zi) (+ drive) -> negatives to 0 ->
    SI_Controlled over [segment, forecast].  seg [L, R] (the last L days of each region's alpha), beta / s0 / i0 [R], dt a
    number; chain = region * D + draw, B = R * D.  z [H, B] standard-normal draws (None = zeros: the deterministic
    continuation); drive [H, Sd] with drive_series [B] (None: Sd == B), added before the clamp: gamma * (u' * a + b).  A
    NumPy drive_series is range-checked on the host; one that is already a device tensor is NOT read back and must hold
    entries in 0 .. Sd-1 (the library trusts it, as it trusts alpha_series).
    A [p, R] (a_1 .. a_p) and noise_var [R] together select the given-model mode (MATLAB's get(ar_sys, 'A')(2:end) and
    'NoiseVariance'); otherwise the model is fitted, with nv_mode 0 = (forward RSS + backward RSS) / (2 (L - p)) or
    1 = forward RSS / (L - p) as its noise variance.  Inputs are torch tensors (taken where they are) or NumPy arrays (copied
    to `device`).  Returns a dict of device tensors: S [L + H, 3, B] with rows (s, i, alpha_hat) -- what
    ensemble_summary(S, R, D, population=N) takes -- A [p, R], noise_var [R], status [R] int32 (_lib.ARFC_OK,
    ARFC_RANK_DEFICIENT: NaN from day L on, ARFC_BAD_INPUT: NaN everywhere).  Enqueued on `stream` (default: the current
    stream) without a host synchronisation.  seed= (and noise_stream=, since `stream` is the HIP stream here): the draws
    normal_draws(H, 1, B, seed, noise_stream)[:, 0] generated inside the kernel; seed and z together raise."""
    noise = _lib.noise_of(seed, noise_stream, z)
    if (A is None) != (noise_var is None):
        raise ValueError("A and noise_var are given together (the given-model mode) or not at all")
    tensors = [v for v in (seg, beta, s0, i0, z, drive, drive_series, A, noise_var) if isinstance(v, torch.Tensor)]
    dev = tensors[0].device if tensors else torch.device(device)

    def put(v, dtype=torch.float64):
        if v is None:
            return None
        if not isinstance(v, torch.Tensor):
            v = torch.as_tensor(np.ascontiguousarray(v, dtype=np.int32 if dtype == torch.int32 else np.float64))
        return v.to(dev, dtype).contiguous()

    seg = put(seg)
    if seg.dim() != 2:
        raise ValueError("seg must be [L, R]")
    L, R = seg.shape
    p, H, D = int(p), int(H), int(D)
    B = R * D
    beta, s0, i0, z, drive, A, noise_var = (put(v) for v in (beta, s0, i0, z, drive, A, noise_var))
    if drive_series is not None and not isinstance(drive_series, torch.Tensor) and drive is not None:
        hs = np.asarray(drive_series)                   # checked on the host, before the upload: no read-back
        if hs.size and (hs.min() < 0 or hs.max() >= np.shape(drive)[-1]):
            raise ValueError("drive_series must hold entries in 0 .. Sd-1")
    ser = put(drive_series, torch.int32)
    for name, v in (("beta", beta), ("s0", s0), ("i0", i0), ("noise_var", noise_var)):
        if v is not None and tuple(v.shape) != (R,):
            raise ValueError(f"{name} must be [R]")
    if z is not None and tuple(z.shape) != (H, B):
        raise ValueError("z must be [H, R * D]")
    if A is not None and tuple(A.shape) != (p, R):
        raise ValueError("A must be [p, R]")
    Sd = 0
    if drive is not None:
        if drive.dim() != 2 or drive.shape[0] != H:
            raise ValueError("drive must be [H, Sd]")
        Sd = drive.shape[1]
        if ser is not None and tuple(ser.shape) != (B,):
            raise ValueError("drive_series must be [R * D]")
    elif ser is not None:
        raise ValueError("drive_series without drive")
    d = _lib.make_arfc_desc(R, D, L, p, H, dt, fit=int(A is None), nv_mode=nv_mode, Sd=Sd)
    ins = _lib.ArfcInputs()
    for k, v in zip(_lib.ARFC_IN_NAMES, (seg, beta, s0, i0, z, drive, ser, A, noise_var)):
        setattr(ins, k, _ptr(v))
    out = _call.run_family("arfc", DeviceBackend(dev, stream), d, [C.byref(ins)], _lib.arfc_shapes(R, D, L, p, H), _lib.ARFC_OUT_NAMES,
                           noise=noise)
    return {"S": out["S"], "A": out["A_out"], "noise_var": out["noise_var_out"], "status": out["status"]}


FUSE_OUTPUTS = ("s", "P", "d2", "rank", "status")


def two_filter(sf, Pf, sb, Pb, form=1, p_solver=0, lane_block=0, outputs=FUSE_OUTPUTS, stream=None, B=None):
    """The forward-backward filter fusion of Tools/TrainPredictPrescribeNPI.m:464-478 for every (chain, day) in one device
    call (epi_fuse_run_device).  sf, sb [T, m, B] and Pf, Pb [T, m*m, B] device tensors, m = 3 or 6, all
    float64 or all float32 -- or, with lane_block = an EkfRunner's `blk`, its chain-blocked outputs [T, nblk, rows, blk] as
    they lie (runner.out["S_PLUS"], ...: nothing is unblocked or copied) with B = the number of chains (default nblk * blk:
    the padding lanes of the last block then count as chains).  The call does not care which filter outputs the
    four are: forward S_PLUS / P_PLUS with backward S_MINUS / P_MINUS counts day t's observation once, PLUS with PLUS is the
    reference's choice.
    form = 1 (the default here; the C ABI has none) is the information form of the two-filter smoother,
        S = Pf + Pb, X = pinv(S):  s = Pb X sf + Pf X sb,  P = Pf X Pb, symmetrised,
    which is what fusing two independent estimates means.  form = 0 is the reference's two lines as written,
        s = X (Pb sf + Pf sb),  P = S \\ (Pf Pb)  (p_solver 0, LU) or X (Pf Pb)  (p_solver 1), not symmetrised;
    they equal form 1 only when Pf, Pb and X commute -- presumably why the reference keeps the block commented out -- and
    are offered for parity with it, not as an estimator.
    A non-finite entry of Pf + Pb (upper triangle), sf or sb gives NaN outputs, rank -1 and bit 0 (_lib.FUSE_NONFINITE) of
    the chain's status; bit 1 (_lib.FUSE_SWEEP_CAP) reports a Jacobi sweep cap.  outputs: any of "s", "P" (same layout and
    dtype as the inputs), "d2" [T, B] float64 (the squared Mahalanobis distance (sf - sb)' X (sf - sb)), "rank" [T, B] int32
    (rank kept by pinv), "status" [B] int32; at least one of s / P / d2.  Returns a dict of device tensors.  Enqueued on
    `stream` (default: the current stream) without a host synchronisation."""
    for name, v in (("sf", sf), ("Pf", Pf), ("sb", sb), ("Pb", Pb)):
        if not isinstance(v, torch.Tensor) or not v.is_cuda:
            raise ValueError(f"{name} must be a device tensor")
        if not v.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if not (sf.dtype == Pf.dtype == sb.dtype == Pb.dtype) or sf.dtype not in (torch.float64, torch.float32):
        raise ValueError("sf, Pf, sb, Pb must all be float64 or all float32")
    if sb.shape != sf.shape or Pb.shape != Pf.shape:
        raise ValueError("sb / Pb must have the shapes of sf / Pf")
    blk = int(lane_block)
    if sf.dim() == 3 and Pf.dim() == 3:
        T, m, nB = sf.shape
        if 0 < blk < nB:
            raise ValueError("lane_block given with classic [T, rows, B] tensors")
        if B is not None and int(B) != nB:
            raise ValueError("B does not match the tensors")
        B, blk = nB, 0
    elif sf.dim() == 4 and Pf.dim() == 4:
        T, nblk, m, bl = sf.shape
        if bl != blk:
            raise ValueError("chain-blocked tensors [T, nblk, rows, blk] need lane_block = blk")
        B = nblk * blk if B is None else int(B)
        if nblk != (B + blk - 1) // blk or blk >= B:
            raise ValueError("B does not match nblk blocks of lane_block chains")
    else:
        raise ValueError("sf / Pf must be [T, m, B] / [T, m*m, B] or [T, nblk, m, blk] / [T, nblk, m*m, blk]")
    if m not in (3, 6) or tuple(Pf.shape) != tuple(sf.shape[:-2]) + (m * m, sf.shape[-1]):
        raise ValueError("m must be 3 or 6 and Pf must hold m*m rows")
    outputs = tuple(outputs)
    for k in outputs:
        if k not in FUSE_OUTPUTS:
            raise ValueError(f"unknown output {k!r}")
    dev = sf.device
    d = _lib.make_fuse_desc(m, B, T, form, p_solver=p_solver, lane_block=blk, storage=int(sf.dtype == torch.float32))
    shapes = _lib.fuse_shapes(m, B, T, blk)
    abi = {"s": "s_out", "P": "P_out", "d2": "d2", "rank": "rank", "status": "status"}
    ins = _lib.FuseInputs()
    for k, v in zip(_lib.FUSE_IN_NAMES, (sf, Pf, sb, Pb)):
        setattr(ins, k, _ptr(v))
    out = _call.run_family("fuse", DeviceBackend(dev, stream), d, [C.byref(ins)], shapes, [abi[k] for k in outputs],
                           f32=("s_out", "P_out") if sf.dtype == torch.float32 else ())
    return {k: out[abi[k]] for k in outputs}


def innovation_likelihood(S_MINUS, P_MINUS, innovations, x, prm, model, R_series=None, R_scalar=None, x_series=None, L=21,
                          obs_type="NEWCASES", k0=0, k1=None, lane_block=0, B=None, G=0, outputs=None, stream=None):
    """The Gaussian innovation log-likelihood of every chain from what a filter run left on the device (epi_loglik_run_device,
    DESIGN.md §4.14): per observed day of the window k0 <= k < k1 (filter steps; k1 = None: T) the innovation variance
    S = C P- C' + gamma R(k) -- the denominator the filter divided by, bit for bit -- and
        loglik = -1/2 sum (log S + e^2 / S + log 2 pi),   nis_mean = mean of e^2 / S.
    It is the likelihood of the EKF's linearisation: with the state clamps and gamma != 1 a score for comparing candidates of
    one region (Q_w, R_v, gamma, beta), not a calibrated probability.
    S_MINUS [T, m, B], P_MINUS [T, m*m, B], innovations [T, B] device tensors of `model`'s run, all float64 or all float32 --
    or, with lane_block = an EkfRunner's `blk`, its chain-blocked outputs [T, nblk, rows, blk] / [T, nblk * blk] as they lie
    (nothing is unblocked or copied) with B = the number of chains.  x [T, Sx], R_series [T, Sx] or R_scalar [B], x_series [B]
    or None, prm [PRM_COUNT, B] and L, obs_type are the filter's own inputs.  With R_scalar the filter's adaptive R(k) is
    replayed from the stored innovations (from float32 ones: bit 2, _lib.LOGLIK_ROUNDED_REPLAY, of the status of every chain
    with beta != 1).  A day whose S is not a normal positive number or whose innovation is not finite is left out and sets
    bit 0 (_lib.LOGLIK_BAD_DAY).
    outputs: any of "loglik", "nis_mean" [B] float64, "n_valid", "status" [B] int32, "S", "nis", "R_used" [T, B] float64 by day
    (NaN where the day does not count; R_used = R(k) on every day), and with G > 0 (B = regions x G chains, region-major)
    "best" [B / G] int32 (the lowest index of the largest loglik among the candidates without a bad day and with n_valid > 0,
    or -1) and "best_loglik" (or NaN).  Default: the four per-chain ones, plus the selection with G > 0.  Returns a dict of
    device tensors.  Enqueued on `stream` (default: the current stream) without a host synchronisation."""
    for name, v in (("S_MINUS", S_MINUS), ("P_MINUS", P_MINUS), ("innovations", innovations)):
        if not isinstance(v, torch.Tensor) or not v.is_cuda:
            raise ValueError(f"{name} must be a device tensor")
        if not v.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if not (S_MINUS.dtype == P_MINUS.dtype == innovations.dtype) or S_MINUS.dtype not in (torch.float64, torch.float32):
        raise ValueError("S_MINUS, P_MINUS, innovations must all be float64 or all float32")
    dev = S_MINUS.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(st):                         # the workspace and the outputs belong to the stream of the call
        return _call.innovation_likelihood(DeviceBackend(dev, st), S_MINUS, P_MINUS, innovations, x, prm, model, R_series, R_scalar,
                                           x_series, L, obs_type, k0, k1, lane_block, B, G, outputs)


def npi_plan(sp, u_min, eps, horizon, u_fixed=None, u_init=None, J0_prefix=None, J1_prefix=None, prefix_days=0, max_iter=64,
             max_halvings=30, tol=1e-9, outputs=None, device="cuda:0"):
    """The direct optimal-NPI planner: a deterministic, well-conditioned optimal plan for every (region, cost weight) chain in
    one device call (epi_plan_run_device).  It solves the Pontryagin problem of the prescription path in its
    stable direction: the horizon simulated forward (the scoring tail's own day), the exact adjoint of the clamped Euler map
    backward from zero, Frank-Wolfe steps u + theta (u* - u) to the bang-bang vertex u* the reference's switching function
    names, theta = 1, 1/2, ... until F = (1 - eps) sum s i alpha + eps sum w'u drops.  It returns a stationary point with its
    Frank-Wolfe gap, not a certificate of global optimality.
    sp [48, R] (pipeline.scoring_region_inputs), u_min [n, R], eps [P] cost weights, horizon H days.  Chain c = region * P + l.
    u_fixed [H, n, R]: NaN = free, a number = held at it (the sweep's convention).  u_init [H, n, R * P]: the starting plan of the
    free entries (default u_min).  J0_prefix, J1_prefix [R] with prefix_days: NPICost's historic sums, as for random_npi_mc.
    Returns a dict of device tensors: plan [H, n, B], J0, J1, F, gap [B] float64, iters, halvings, status [B] int32 (status 0:
    gap <= tol |F|; _lib.PLAN_STOP_CAP: max_iter adjoint passes without it; _lib.PLAN_STOP_SEARCH: no descending step;
    _lib.PLAN_STOP_NONFINITE: F not finite), and those of outputs = ("states", "mu", "F_trace") asked for: states, mu [H, 3, B]
    of the plan returned, F_trace [max_iter, B] (NaN beyond iters; strictly decreasing).  Enqueued on the current stream
    without a host synchronisation."""
    return _call.npi_plan(DeviceBackend(device), sp, u_min, eps, horizon, u_fixed, u_init, J0_prefix, J1_prefix, prefix_days, max_iter,
                          max_halvings, tol, outputs)


def smoother_draws(S_PLUS, P_PLUS, S_MINUS, P_MINUS, prm, D, z=None, s_term=None, P_term=None, k0=0, clamp=True, lane_block=0, B=None,
                   out_dtype=None, outputs=("X", "rank", "status"), stream=None, seed=None, noise_stream=0):
    """Joint posterior draws of the smoothed paths by backward simulation, from what a 3-state filter run left on the device
    (epi_sdraw_run_device): D paths per chain of the law whose mean and covariance recursions are the
    smoother's own (GenericExtendedKalmanFilter.m:218, :223),
        x_T = clamp(s_T + F_T z_T),   x_k = clamp((S+_k + J_k (x_{k+1} - S-_{k+1})) + F_k z_k),   k = T-1 ... k0,
    J_k the smoother's gain, F_k the pivoted Cholesky factor of P+_k - J_k P-_{k+1} J_k'.  Path p = chain * D + draw, so X is
    what ensemble_summary(X, B, D) takes.
    S_PLUS, S_MINUS [T, 3, B], P_PLUS, P_MINUS [T, 9, B] device tensors of a SIAlphaModelEKF run, all float64 or all float32 --
    or, with lane_block = an EkfRunner's `blk`, its chain-blocked outputs [T, nblk, rows, blk] as they lie (nothing is unblocked
    or copied) with B = the number of chains.  prm [PRM_COUNT, B] the filter's own.  z [T - k0, 3, B * D] standard-normal inputs,
    float64 or float32, or None: no noise term -- with clamp the path is then S_SMOOTH bit for bit.  s_term [3, B], P_term [9, B]:
    the terminal law (the last day of S_SMOOTH / P_SMOOTH when s_final / Ps_final were set; default S_PLUS, P_PLUS of day T-1).
    k0: the first day returned.  clamp: StateHardMargins on every draw (a NaN stays NaN); False: an exactly Gaussian law.
    out_dtype: torch.float64 (default) or torch.float32 for X (the float64 result rounded once).
    outputs: any of "X" [T - k0, 3, B * D], "rank" [T, B] int32 (columns of F kept; -1: a NaN record), "status" [B] int32 (bit 0,
    _lib.SDRAW_NONFINITE: a non-finite input entry met -- J = 0 by the guard :211, or a NaN record; bit 1,
    _lib.SDRAW_RANK_DEFICIENT: a rank below 3 on some day), "J", "L" [T, 9, B] float64 (entry i + 3 j; L = F, a row-permuted lower
    triangle).  Returns a dict of device tensors.  Enqueued on `stream` (default: the current stream) without a host
    synchronisation.  seed= (and noise_stream=, since `stream` is the HIP stream here): the draws normal_draws(T - k0, 3, B * D,
    seed, noise_stream) generated inside the kernel -- no z array exists; seed and z together raise."""
    for name, v in (("S_PLUS", S_PLUS), ("P_PLUS", P_PLUS), ("S_MINUS", S_MINUS), ("P_MINUS", P_MINUS)):
        if not isinstance(v, torch.Tensor) or not v.is_cuda:
            raise ValueError(f"{name} must be a device tensor")
        if not v.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if not (S_PLUS.dtype == P_PLUS.dtype == S_MINUS.dtype == P_MINUS.dtype) or S_PLUS.dtype not in (torch.float64, torch.float32):
        raise ValueError("S_PLUS, P_PLUS, S_MINUS, P_MINUS must all be float64 or all float32")
    dev = S_PLUS.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(st):                         # the workspace and the outputs belong to the stream of the call
        return _call.smoother_draws(DeviceBackend(dev, st), S_PLUS, P_PLUS, S_MINUS, P_MINUS, prm, D, z, s_term, P_term, k0, clamp,
                                    lane_block, B, out_dtype, outputs, 0, seed, noise_stream)


def ensemble_score(src, truth, R, D, alpha=_lib.ESCORE_DEFAULT_ALPHA, n_bins=0, population=None, truth_series=None, first_day=None,
                   k0=0, k1=None, outputs=None, stream=None, test_launch_items=0):
    """Probabilistic forecast scores of a Monte-Carlo ensemble against a truth in one device call (epi_escore_run_device,
    DESIGN.md §4.17).  src [T, rows, B] or [T, B] (float32 or float64, on the device) is what ensemble_summary takes: B = R * D
    chains, region-major; population [R] appends the derived new-case row.  truth [T, rows', Rt] ([T, Rt] for a [T, B] src): the
    truth of item (t, row, r) is truth[t, row, truth_series[r]] (truth_series [R] int32; None: Rt = R and column r).  NaN members
    are absent; an item without members or with a NaN truth is not scored.
    alpha: up to 8 levels of central intervals, each in (0, 1), strictly descending (0.5, 0.05: the 50 % and the 95 % band).
    Per item [T, rows', R]: crps (the ensemble CRPS), wis (the weighted interval score of the median and the intervals), ae
    (|truth - median|), rank, ties (members below / equal to the truth), cover (bit k: the truth lies in interval k), count
    (int32), and width [T, n_a, rows', R].  Per (row, region) over the days k0 <= t < k1 (k1 = None: T) from first_day[r] on
    (first_day [R] int32, the forecast origin of every region): crps_mean, wis_mean, ae_mean, n_scored [rows', R], cover_frac
    [n_a, rows', R], and with n_bins > 0 (at most 32) pit_hist [n_bins, rows', R], the histogram of the non-randomised mid-rank.
    outputs: any of these names (default: all).  Returns a dict of device tensors.  Enqueued on `stream` (default: the current
    stream) without a host synchronisation.  A chain-blocked output (EkfRunner(lane_block=...)) is not accepted.
    test_launch_items: the tests' launch cut (0 in production)."""
    if not isinstance(src, torch.Tensor):
        raise TypeError("src must be a torch tensor (NumPy arrays: hostapi.ensemble_score)")
    if src.dim() == 4:
        raise ValueError("src is a chain-blocked tensor [T, nblk, rows, blk]; ensemble_score takes the classic layout "
                         "[T, rows, B]: pass EkfRunner.unblocked(name).contiguous(), or run with lane_block=0")
    if src.dtype not in (torch.float32, torch.float64):
        raise TypeError("src must be float32 or float64")
    dev = src.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(st):                         # the workspace and the outputs belong to the stream of the call
        return _call.ensemble_score(DeviceBackend(dev, st), src.contiguous(), truth, R, D, alpha, n_bins, population, truth_series,
                                    first_day, k0, k1, outputs, test_launch_items)


def path_functionals(src, R, D, thresholds=None, population=None, first_day=None, k0=0, k1=None, outputs=None, stream=None,
                     test_segments=0, test_launch_groups=0):
    """Functionals of every joint path of a Monte-Carlo ensemble in one device call (epi_pathfn_run_device): one
    streaming read of src answers when the peak is, how high, how many cases over the window, and when, for how many days and
    for how long a threshold is exceeded.  src [T, rows, B] or [T, B] (float32 or float64, on the device) is what
    ensemble_summary takes: B = R * D paths, region-major; population [R] appends the derived new-case row.  The window is the
    days k0 <= t < k1 (k1 = None: T), for region r from first_day[r] on (first_day [R] int32); a NaN value is no day of its path.
    thresholds [n_thr, rows', R] (at most 8; [n_thr, R] for a [T, B] src): a NaN entry asks nothing of that row and region.
    Per path [rows', B], float64 (each is itself an ensemble_summary source): peak_value, peak_day (the first day of the maximum,
    the day index of src), min_value, min_day, total (the sum in 32-day blocks); per threshold [n_thr, rows', B]: first_cross
    (NaN: never), days_above, longest_run; n_valid (int32).  A path without a valid day is NaN throughout.  Per (row, region)
    over the paths with a valid day, int32: n_paths [rows', R], peak_day_hist [W, rows', R] (bin t - k0), n_cross [n_thr, rows',
    R], cross_day_hist [W, n_thr, rows', R] (W = k1 - k0, at most 4096 for a histogram).
    outputs: any of these names (default: all).  Returns a dict of device tensors.  Enqueued on `stream` (default: the current
    stream) without a host synchronisation.  A chain-blocked output (EkfRunner(lane_block=...)) is not accepted.
    test_segments, test_launch_groups: the tests' time segments and launch cut (0 in production)."""
    if not isinstance(src, torch.Tensor):
        raise TypeError("src must be a torch tensor (NumPy arrays: hostapi.path_functionals)")
    if src.dim() == 4:
        raise ValueError("src is a chain-blocked tensor [T, nblk, rows, blk]; path_functionals takes the classic layout "
                         "[T, rows, B]: pass EkfRunner.unblocked(name).contiguous(), or run with lane_block=0")
    if src.dtype not in (torch.float32, torch.float64):
        raise TypeError("src must be float32 or float64")
    dev = src.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(st):                         # the workspace and the outputs belong to the stream of the call
        return _call.path_functionals(DeviceBackend(dev, st), src.contiguous(), R, D, thresholds, population, first_day, k0, k1,
                                      outputs, test_segments, test_launch_groups)


def curve_statistics(src, R, D, alpha=_lib.CDEPTH_DEFAULT_ALPHA, fence_factor=_lib.CDEPTH_DEFAULT_FENCE_FACTOR,
                     fence_frac=_lib.CDEPTH_DEFAULT_FENCE_FRAC, population=None, first_day=None, k0=0, k1=None, outputs=None, stream=None,
                     test_segments=0, test_launch_groups=0):
    """Statistics of the CURVES of a Monte-Carlo ensemble in one device call (epi_cdepth_run_device): which path
    is the typical one, and what band the central fraction of the paths covers -- what a per-day quantile cannot say, since a
    per-day band is made of no curve and flattens a peak that the members reach on different days.  src [T, rows, B] or [T, B]
    (float32 or float64, on the device) is what ensemble_summary takes: B = R * D paths, region-major; population [R] appends
    the derived new-case row.  The window is the days k0 <= t < k1 (k1 = None: T), for region r from first_day[r] on (first_day
    [R] int32); a NaN value is no day of its path.
    Per path [rows', B]: depth, the modified band depth with bands of two curves (the share of (pair of members, day) whose band
    holds the path; NaN for a path without a day that has two members), mhi (the modified hypograph index: the share of
    (member, day) at or below the path), band_count and pair_total (depth's exact integer numerator and denominator), float64
    and each itself an ensemble_summary source; n_valid, depth_rank (0 the deepest of its region, the lower draw wins a tie, -1
    unranked), out_days (the days outside the fences), int32.  Per (row, region) [rows', R] int32: n_ranked, median_path (the
    draw of rank 0, -1: none), n_outliers (ranked paths with out_days > 0).  Per day: env_lo, env_hi [T, n_alpha, rows', R], the
    envelope of the ceil(alpha n_ranked) deepest paths (alpha: up to 8 fractions in (0, 1], strictly ascending); median_curve [T,
    rows', R], the deepest path; whisk_lo, whisk_hi [T, rows', R], the envelope of the ranked paths that stay inside the fences
    (the envelope of the fence_frac deepest, widened by fence_factor times its width on either side: the functional boxplot).
    Days outside the window are NaN.  fence_factor = 0 or None: no boxplot.
    outputs: any of these names (default: all).  Returns a dict of device tensors.  Enqueued on `stream` (default: the current
    stream) without a host synchronisation.  A chain-blocked output (EkfRunner(lane_block=...)) is not accepted.
    test_segments, test_launch_groups: the tests' time segments and launch cut (0 in production)."""
    if not isinstance(src, torch.Tensor):
        raise TypeError("src must be a torch tensor (NumPy arrays: hostapi.curve_statistics)")
    if src.dim() == 4:
        raise ValueError("src is a chain-blocked tensor [T, nblk, rows, blk]; ensemble_summary takes the classic layout "
                         "[T, rows, B]: pass EkfRunner.unblocked(name).contiguous(), or run with lane_block=0")
    if src.dtype not in (torch.float32, torch.float64):
        raise TypeError("src must be float32 or float64")
    dev = src.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(st):                         # the workspace and the outputs belong to the stream of the call
        return _call.curve_statistics(DeviceBackend(dev, st), src.contiguous(), R, D, alpha, fence_factor, fence_frac, population,
                                      first_day, k0, k1, outputs, test_segments, test_launch_groups)


def ensemble_joint_score(src, truth, R, D, vs_p=None, max_lag=0, population=None, truth_series=None, first_day=None, k0=0, k1=None,
                         outputs=None, stream=None, test_launch_tiles=0):
    """Joint (multivariate) scores of a Monte-Carlo ensemble's paths against a truth in one device call (epi_ejoint_run_device,
    DESIGN.md §4.20): what tells joint draws from draws with the same marginals and no dependence between days, which
    ensemble_score cannot.  src, truth, population, truth_series and first_day are ensemble_score's: src [T, rows, B] or [T, B]
    (float32 or float64, on the device), B = R * D chains, region-major; truth [T, rows', Rt].  An item is one (row, region); its
    days are the t in [max(k0, first_day[r]), k1) (k1 = None: T) whose truth is not NaN, its members the draws without a NaN on
    any of those days.  Per item [rows', R]: es, the energy score (1/n) sum ||x_i - y|| - (1/(2 n^2)) sum sum ||x_i - x_j|| over the
    days (with one day: the CRPS), its two terms truth_term and spread_term, n_members, n_days (int32) and, with vs_p = 0.5 or 1,
    vs: the variogram score of order p over the pairs of days at most max_lag calendar days apart (0: every pair).  member_dist
    [rows', R * D]: every member's distance to the truth (NaN for absent members), itself an ensemble_summary source.  An item
    without members or days gives NaN (its counts are still written).
    outputs: any of these names (default: all, vs only with vs_p).  Returns a dict of device tensors.  Enqueued on `stream`
    (default: the current stream) without a host synchronisation.  A chain-blocked output (EkfRunner(lane_block=...)) is not
    accepted.  test_launch_tiles: the tests' launch cut (0 in production)."""
    if not isinstance(src, torch.Tensor):
        raise TypeError("src must be a torch tensor (NumPy arrays: hostapi.ensemble_joint_score)")
    if src.dim() == 4:
        raise ValueError("src is a chain-blocked tensor [T, nblk, rows, blk]; ensemble_score takes the classic layout "
                         "[T, rows, B]: pass EkfRunner.unblocked(name).contiguous(), or run with lane_block=0")
    if src.dtype not in (torch.float32, torch.float64):
        raise TypeError("src must be float32 or float64")
    dev = src.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(st):                         # the workspace and the outputs belong to the stream of the call
        return _call.ensemble_joint_score(DeviceBackend(dev, st), src.contiguous(), truth, R, D, vs_p, max_lag, population, truth_series,
                                          first_day, k0, k1, outputs, test_launch_tiles)


def innovation_diagnostics(innovations, S=None, n_lags=10, k0=0, k1=None, flip=False, lane_block=0, B=None, outputs=None, stream=None):
    """Whiteness diagnostics of the innovations of every chain in one device call (epi_idiag_run_device): is
    the filter run statistically consistent -- serially uncorrelated, homoskedastic, Gaussian, of unit variance -- over the
    window k0 <= k < k1 of filter steps (k1 = None: T)?
    innovations [T, B] device tensor, float64 or float32 -- or, with lane_block = an EkfRunner's `blk` and B = the number of
    chains, its chain-blocked [T, nblk * blk] as it lies.  S [T, B] float64 by day, exactly innovation_likelihood's output "S"
    (NaN: the day does not count), or None: the innovations are taken as already standardised (e = NaN: the day does not
    count), which makes the call usable on any residual series.  flip: filter step k is row T-1-k (the backward models).
    nu = e / sqrt(S).  A day inside the window whose S is not a normal positive number or whose innovation is not finite is
    left out and sets bit 0 of status (_lib.IDIAG_BAD_DAY).
    outputs: any of, [B] float64, "mean", "var", "skew", "kurt" (of nu; Gaussian: 0, 1, 0, 3), "jb" (Jarque-Bera, chi2 with 2
    degrees of freedom), "nis_sum" (sum of nu^2: chi2 with n degrees of freedom), "nis_mean", "lb_q" (Ljung-Box over lb_lags
    lags, chi2 with lb_lags degrees of freedom), "het" (mean nu^2 of the last third of the window over that of the first: F with
    (het_n2, het_n1) degrees of freedom), "cusumsq_max" (largest |CUSUM of squares| and "cusumsq_step", the step where the
    variance breaks most), "max_abs" (the largest |nu|, at "max_abs_step"); [B] int32 "n" (days that count), "lb_lags" =
    min(n_lags, n - 1), "het_n1", "het_n2", "cusumsq_step", "max_abs_step", "status" (bit 1 IDIAG_EMPTY: n = 0, everything NaN
    / 0 / -1; bit 2 IDIAG_DEGENERATE: no variance, "acf", "skew", "kurt", "jb", "lb_q" NaN; bit 3 IDIAG_FEW_LAGS: lb_lags <
    n_lags); and "acf" [n_lags, B] float64, the autocorrelations of lags 1 .. n_lags.  n_lags 0 .. 64.  Default: all of them.
    Every sum runs in a pinned order, so the bits are reproducible.  Returns a dict of device tensors.  Enqueued on `stream`
    (default: the current stream) without a host synchronisation."""
    for name, v in (("innovations", innovations),) + ((("S", S),) if S is not None else ()):
        if not isinstance(v, torch.Tensor) or not v.is_cuda:
            raise ValueError(f"{name} must be a device tensor")
        if not v.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if innovations.dtype not in (torch.float64, torch.float32):
        raise ValueError("innovations must be float64 or float32")
    if S is not None and S.dtype != torch.float64:
        raise ValueError("S must be float64")
    dev = innovations.device
    st = torch.cuda.current_stream(dev) if stream is None else stream
    with torch.cuda.stream(st):                         # the workspace and the outputs belong to the stream of the call
        return _call.innovation_diagnostics(DeviceBackend(dev, st), innovations, S, n_lags, k0, k1, flip, lane_block, B, outputs)
