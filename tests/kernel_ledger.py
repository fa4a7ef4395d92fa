"""Which test call runs which kernel instance of the filter families -- as a table that is checked, not as comments.

Every row is one call of epi_ekf_run_device (or of the sweep entry): a workload recipe, the EkfRunner arguments with an explicit
integer lane_block, the entry point, and what the row DECLARES: the kernel instances the call launches and its schedule bits on
a device with S_LEDGER SIMDs (MI355X: 256 CUs x 4).  tests/test_kernel_ledger.py (no GPU) asks the launch plan
(tests/plan_query.cpp) whether the declarations hold and whether the rows together reach every instance a plan can launch;
tests/test_gpu_kernel_ledger.py runs every row against the C oracle, bit for bit, after asking the plan again with the
device's own SIMD count.

Names are those `nm -C` prints for the kernels' host stubs; "{F}" stands for the FLIP template argument (0: forward model, 1: the
time-flipped wrapper) and "{M}" for the state count.  `second` lists what the dense second pass of exact_nonfinite launches
(rerun_nonfinite_dense: it does work only for chains whose status marks a covariance overflow); rows with guard=True hold such a
chain, and the GPU test asserts that its guard fired."""
import numpy as np

from tests.test_gpu_npi_counts import SIA6_LAUNCHES

S_LEDGER = 1024          # SIMDs the declarations are made for

FAMILIES = ("ekf_fwd", "eks_bwd", "ekf_monitor", "eks_pinv")     # prefixes: forward, smoother, monitor, the dense pair, the pinv grid

# compiled (the ladder of enqueue_fwd names them) but never launched: the plan sets V_LP (LDS-resident model constants) for
# the 6-state models only.  A condition, not a budget: tests/test_kernel_ledger.py asserts the list is exactly these six.
NEVER_LAUNCHED = ["ekf_fwd_sym<3, %d, 1, %s>" % (f, t) for f in (0, 1) for t in ("0, 0, 0", "0, 0, 1", "0, 1, 0")]


def chains_beyond(waves_chains, n_eps):
    """(n_regions, n_eps) of the smallest regions x n_eps batch with more than waves_chains * S_LEDGER chains."""
    return -(-(waves_chains * S_LEDGER + 1) // n_eps), n_eps


# ---------------------------------------------------------------- workloads
def _flip_row3(w):
    """make_row3 routed to the time-flipped wrapper: it starts from (s_final, Ps_final), which must be finite -- the forward
    start state with zero costates and the forward initial covariance."""
    out = w.select(np.arange(w.B))
    out.model = "SIAlphaModelBackwardEKFOptControlled"
    out.s_final = w.s_init.copy()
    out.s_final[3:] = 0.0
    out.Ps_final = w.Ps_init.copy()
    return out


def _with_offdiag_q(w):
    w = w.select(np.arange(w.B))
    w.Q = w.Q.copy()
    m = w.m
    w.Q[1] = 1e-13
    w.Q[m] = 1e-13
    return w


def _overflowing(w, chain=7):
    """One chain driven into covariance overflow in mid-run (test_mid_run_covariance_overflow_on_the_packed_path): the second
    pass of exact_nonfinite then has a chain to run."""
    w = w.select(np.arange(w.B))
    if "Backward" in w.model:           # (the flipped costate map shrinks that variance: a process noise that overflows on the second day)
        w.Q = w.Q.copy()
        w.Q[0, chain] = 1.7e308
    else:
        w.Ps_init = w.Ps_init.copy()
        w.Ps_init[5 * 6 + 5, chain] = 1e305
    return w


def _huge_q(w, chain=2):
    """3-state: a finite process noise (the precheck keeps the batch on the packed kernels) that makes P(k|k-1) overflow on the
    second day."""
    w = w.select(np.arange(w.B))
    w.Q = w.Q.copy()
    w.Q[0, chain] = 1.7e308
    return w


def _recipes():
    from epidemicmodeling_amd import synth
    cfg4, cfg3, row3 = synth.make_cfg4, synth.make_cfg3, synth.make_row3
    back = synth.as_backward
    r = {
        # the workloads of SIA6_LAUNCHES (tests/test_gpu_npi_counts.py), at 12 NPIs
        "b80": lambda f: back(cfg4(4, 20, 30, 10)) if f else cfg4(4, 20, 30, 10),
        "b70": lambda f: r["b80"](f).select(np.arange(70)),
        "dense": lambda f: _with_offdiag_q(r["b80"](f)),
        "long": lambda f: back(cfg4(2, 20, 120, 10)) if f else cfg4(2, 20, 120, 10),
        "b80-overflow": lambda f: _overflowing(r["b80"](f)),
        "b80-L5": lambda f: _with_L(r["b80"](f), 5),
        "b80-L50": lambda f: _with_L(r["b80"](f), 50),
        # a scalar adaptive R_v: 80 and 70 chains x 40 days
        "row3-b80": lambda f: _flip_row3(row3(4, 20, 30, 10)) if f else row3(4, 20, 30, 10),
        "row3-b70": lambda f: r["row3-b80"](f).select(np.arange(70)),
        "row3-b80-L5": lambda f: _with_L(r["row3-b80"](f), 5),
        # the fp32, 3-state and NewCase calls of tests/test_gpu_npi_counts.py
        "f32-cfg4": lambda f: back(cfg4(3, 10, 30, 8)) if f else cfg4(3, 10, 30, 8),
        "f32-cfg3": lambda f: back(cfg3(30, 36)) if f else cfg3(30, 36),
        "cfg3-23": lambda f: cfg3(23, 40),
        "cfg5-40": lambda f: synth.make_cfg5(2, 20, 36),
        "cfg3-15": lambda f: back(cfg3(15, 30)) if f else cfg3(15, 30),
        "cfg3-dense": lambda f: _with_offdiag_q(r["cfg3-15"](f)),
        "cfg3-overflow": lambda f: _huge_q(r["cfg3-15"](f)),
        "cfg3-L5": lambda f: _with_L(r["cfg3-15"](f), 5),
        "cfg3-L50": lambda f: _with_L(r["cfg3-15"](f), 50),
        "row4": lambda f: synth.make_row4(7, 40, 12, codegen=False),
        "row4-codegen": lambda f: synth.make_row4(7, 40, 12, codegen=True),
        "row4-L5": lambda f: _with_L(synth.make_row4(7, 40, 12), 5),
        # beyond 64 chains per SIMD (one round of 64-lane waves): the forward kernel narrows its waves to 40 lanes (LP, USD)
        "lp": lambda f: back(cfg4(*chains_beyond(64, 16), 4, 2)) if f else cfg4(*chains_beyond(64, 16), 4, 2),
        "lp-row3": lambda f: _flip_row3(row3(*chains_beyond(64, 16), 4, 2)) if f else row3(*chains_beyond(64, 16), 4, 2),
        "lp-sweep": lambda f: cfg4(*chains_beyond(64, 40), 5, 3),
        # beyond one hex wavefront (10 chains) / one quad wavefront (16 chains) per SIMD
        "hex2": lambda f: back(cfg4(*chains_beyond(10, 121), 4, 2)) if f else cfg4(*chains_beyond(10, 121), 4, 2),
        "quad2": lambda f: back(cfg4(*chains_beyond(16, 125), 4, 2)) if f else cfg4(*chains_beyond(16, 125), 4, 2),
        # the sweep entry at 80 chains (test_sweep_entry_every_npi_count)
        "sweep80": lambda f: cfg4(2, 40, 30, 11),
    }
    return r


def _with_L(w, L_):
    w = w.select(np.arange(w.B))
    w.L = L_
    return w


_made = {}


def workload(name, flipped):
    """The Workload of a row (made once per process; treat it as read-only)."""
    key = (name, bool(flipped))
    if key not in _made:
        _made[key] = _recipes()[name](bool(flipped))
    return _made[key]


# ---------------------------------------------------------------- rows
RUNNER_DEFAULTS = dict(shape="auto", lane_block=0, outputs=None, storage="f64", time_pipe=0, test_window=0, test_flags=0)
SECOND = ["ekf_fwd<{M}, {F}, 1>", "eks_pinv<{M}, 1>", "eks_bwd<{M}, {F}, 1>"]       # the dense second pass of a generic model
OV = "OVERLAP"
PINV, PAR = "eks_pinv<{M}, 0>", "ekf_monitor_par<{F}, 21, 8>"


def _row(id, wl, names, sched, flips=(0, 1), hint=1, second=SECOND, entry="run", t_hist=None, guard=False, bwd_order=None, fwd_lds=None, **runner):
    out = []
    for f in flips:
        w_m = 3 if wl.startswith(("cfg3", "cfg5", "f32-cfg3")) else 6
        sub = lambda l: sorted(n.format(F=f, M=w_m) for n in l)
        kw = dict(RUNNER_DEFAULTS)
        kw.update(runner)
        assert isinstance(kw["lane_block"], int)
        out.append(dict(id="%s/%s" % (id, "flipped" if f else "forward"), workload=wl, flipped=bool(f), runner=kw, entry=entry, t_hist=t_hist,
                        hint=hint, names=sub(names), second=sub(second), schedule=sched, guard=guard, fwd_lds=fwd_lds,
                        bwd_order=None if bwd_order is None else [n.format(F=f, M=w_m) for n in bwd_order]))
    return out


def _sym(lp=0, stor=0, mon=0, usd=0):
    return "ekf_fwd_sym<{M}, {F}, %d, %d, %d, %d>" % (lp, stor, mon, usd)


FWD_SYM, BWD_SYM = _sym(), "eks_bwd_sym<{M}, {F}, 0>"
L6 = "eks_bwd_lane6<{F}, %d, %d>"
DENSE = ["ekf_fwd<{M}, {F}, 1>", "eks_bwd<{M}, {F}, 1>"]

# what each row of SIA6_LAUNCHES launches (the comments of tests/test_gpu_npi_counts.py as declarations): (names, schedule)
_SIA6_DECLARED = {
    "lane-classic": ([FWD_SYM, BWD_SYM, PINV, PAR], OV),
    "lane-blk8": ([FWD_SYM, BWD_SYM, PINV, PAR], OV),
    "lane-blk48": ([FWD_SYM, L6 % (48, 0), PINV, PAR], OV),
    "lane-blk56": ([FWD_SYM, L6 % (56, 0), PINV, PAR], OV),
    "lane-blk40-xd": ([FWD_SYM, L6 % (40, 1), PINV, PAR], OV),
    "lane-blk40-ragged": ([FWD_SYM, L6 % (40, 0), PINV, PAR], OV),
    "lane-blk40-split": ([FWD_SYM, L6 % (40, 1), PINV, PAR], "OVERLAP|FWD_RANGES|BWD_ROUNDS"),
    "lane-blk40-window2": ([FWD_SYM, L6 % (40, 1), PINV, PAR], OV),
    "quad-classic": (["ekf_fwd_quad<{F}, 0, 0, 0, 1>", "eks_bwd_quad<{F}, 0>", PINV, PAR], OV),
    "quad-blk16": (["ekf_fwd_quad<{F}, 16, 21, 0, 1>", "eks_bwd_quad<{F}, 16>", PINV, PAR], OV),
    "wave": (["ekf_fwd_wave<{F}, 0, 0, 1>", "eks_bwd_wave<{F}>", PINV, PAR], OV),
    "hex-blk10": (["ekf_fwd_hex<{F}, 10, 1>", "eks_bwd_hex<{F}, 10, 2>", PINV, PAR], OV),
    "hex-classic-window4": (["ekf_fwd_hex<{F}, 0, 1>", "eks_bwd_hex<{F}, 0, 1>", PINV, PAR], OV),
    "hex-reverse-pipe": (["ekf_fwd_hex<{F}, 10, 1>", "eks_bwd_hex<{F}, 10, 2>", PINV, PAR], "OVERLAP|REVERSE_PIPE"),
    # path_hint = 2: one stage after the other, the monitor inside the dense forward kernel, no second pass
    "dense": (DENSE + [PINV], ""),
    "time-pipe": ([FWD_SYM, L6 % (40, 1), PINV, PAR], "OVERLAP|TIME_PIPE"),
    "reduced-u-blk40": ([FWD_SYM, L6 % (40, 1), PINV], OV),
    "reduced-3-classic": ([FWD_SYM, BWD_SYM, PINV, PAR], OV),
}


def _rows():
    rows = []
    for name, wl, kw in SIA6_LAUNCHES:
        names, sched = _SIA6_DECLARED[name]
        kw = dict(kw)
        kw.setdefault("lane_block", 0)
        rows += _row("sia6/" + name, wl, names, sched, hint=2 if wl == "dense" else 1, second=[] if wl == "dense" else SECOND, **kw)
    # ---- the fp32, 3-state and NewCase calls of tests/test_gpu_npi_counts.py
    for blk in (0, 8):
        for wl in ("f32-cfg4", "f32-cfg3"):
            rows += _row("f32/%s-blk%d" % (wl[4:], blk), wl, [_sym(stor=1), "eks_bwd_sym<{M}, {F}, 1>", PINV, PAR], OV, second=[],
                         storage="f32", shape="lane", lane_block=blk)
    for wl, flips in (("cfg3-23", (0,)), ("cfg5-40", (0,)), ("cfg3-15", (1,))):
        for blk in (0, 8):
            rows += _row("sia3/%s-lane-blk%d" % (wl, blk), wl, [FWD_SYM, BWD_SYM, PINV, PAR], OV, flips=flips, shape="lane", lane_block=blk)
        for blk in (0, 7):
            rows += _row("sia3/%s-wave3-blk%d" % (wl, blk), wl, ["ekf_fwd_wave3<{F}>", "eks_bwd_wave3<{F}>", PINV, PAR], OV, flips=flips,
                         shape="wave", lane_block=blk)
    for wl in ("row4", "row4-codegen"):
        rows += _row("newcase/%s-dense" % wl, wl, ["ekf_fwd<6, 0, 0>", "eks_bwd<6, 0, 0>"], "", flips=(0,), hint=2, second=[], shape="lane")
        for blk in (0, 8):
            rows += _row("newcase/%s-wave-blk%d" % (wl, blk), wl, ["ekf_fwd_wave<0, 1, 21, 0>", "eks_bwd_wave_nc"], "", flips=(0,), hint=2,
                         second=[], shape="wave", lane_block=blk)
    # ---- more chains than one round of 64-lane waves (64 S): 40-lane waves, the forward kernel with its constants in LDS (LP)
    big = "OVERLAP|FWD_RANGES|BWD_ROUNDS"
    # (the smoother's first launch holds whole 40-chain blocks: XD = 1; the second ends in a ragged block: XD = 0)
    rows += _row("lp/blk40-all", "lp", [_sym(lp=1), L6 % (40, 1), L6 % (40, 0), PINV, PAR], big, lane_block=40, bwd_order=[L6 % (40, 1), L6 % (40, 0)])
    rows += _row("lp/classic-all", "lp", [_sym(lp=1), BWD_SYM, PINV, PAR], "OVERLAP|FWD_RANGES")
    rows += _row("lp/classic-usd", "lp", [_sym(lp=1, usd=1), BWD_SYM, PINV], OV, outputs=["S_SMOOTH", "u_opt_smooth"])
    # (no hoisted monitor to put between two smoother launches: ONE launch, and B is not a multiple of 40, so XD = 0)
    rows += _row("lp/blk40-inline-monitor", "lp-row3", [_sym(lp=1, mon=1), L6 % (40, 0), PINV], "OVERLAP|FWD_RANGES", lane_block=40, fwd_lds=35520)
    rows += _row("lp/sweep-blk40", "lp-sweep", [_sym(lp=1), L6 % (40, 1), PINV, PAR], big, flips=(0,), entry="sweep", t_hist=5, lane_block=40)
    # ---- the hex shape beyond one wavefront per SIMD (10 S chains): two waves per SIMD, no prefetch set in the smoother
    for f in (0, 1):
        rows += _row("hex2/blk10", "hex2", ["ekf_fwd_hex<{F}, 10, 0>", "eks_bwd_hex<{F}, 10, 0>", PINV, PAR], OV, flips=(f,), lane_block=10)
        rows += _row("hex2/classic", "hex2", ["ekf_fwd_hex<{F}, 0, 0>", "eks_bwd_hex<{F}, 0, 0>", PINV, PAR], OV, flips=(f,))
        rows += _row("hex2/blk10-reverse-pipe", "hex2", ["ekf_fwd_hex<{F}, 10, 0>", "eks_bwd_hex<{F}, 10, 0>", PINV, PAR], "OVERLAP|REVERSE_PIPE",
                     flips=(f,), lane_block=10, test_flags=1)
    # ---- the quad shape beyond one wavefront per SIMD (16 S chains), forced
    rows += _row("quad2/classic", "quad2", ["ekf_fwd_quad<{F}, 0, 0, 0, 0>", "eks_bwd_quad<{F}, 0>", PINV, PAR], OV, shape="quad")
    rows += _row("quad2/blk16", "quad2", ["ekf_fwd_quad<{F}, 16, 21, 0, 0>", "eks_bwd_quad<{F}, 16>", PINV, PAR], OV, shape="quad", lane_block=16)
    # ---- a scalar adaptive R_v (the forward kernel keeps its monitor) on the layouts of eks_bwd_lane6
    for blk in (40, 48, 56):
        rows += _row("row3/b80-blk%d" % blk, "row3-b80", [_sym(mon=1), L6 % (blk, 1 if blk == 40 else 0), PINV], OV, shape="lane", lane_block=blk)
        rows += _row("row3/b70-blk%d" % blk, "row3-b70", [_sym(mon=1), L6 % (blk, 0), PINV], OV, shape="lane", lane_block=blk)
    # ---- what else no row above reaches
    # inline monitor on the other shapes (scalar R_v), and window lengths other than the 21 the specialisations are compiled for
    rows += _row("row3/quad-classic", "row3-b80", ["ekf_fwd_quad<{F}, 0, 0, 1, 0>", "eks_bwd_quad<{F}, 0>", PINV], OV, shape="quad")
    rows += _row("row3/quad-blk16", "row3-b80", ["ekf_fwd_quad<{F}, 16, 21, 1, 0>", "eks_bwd_quad<{F}, 16>", PINV], OV, shape="quad", lane_block=16)
    rows += _row("row3/wave", "row3-b80", ["ekf_fwd_wave<{F}, 1, 21, 1>", "eks_bwd_wave<{F}>", PINV], OV, shape="wave")
    rows += _row("row3/wave-L5", "row3-b80-L5", ["ekf_fwd_wave<{F}, 1, 0, 1>", "eks_bwd_wave<{F}>", PINV], OV, shape="wave")
    rows += _row("newcase/wave-L5", "row4-L5", ["ekf_fwd_wave<0, 1, 0, 0>", "eks_bwd_wave_nc"], "", flips=(0,), hint=2, second=[], shape="wave")
    # L != 21 (and test_flags bit 1) take the scanning monitor; L = 50: the windows no longer fit beside a hoisted monitor
    rows += _row("sia6/lane-L5", "b80-L5", [FWD_SYM, BWD_SYM, PINV, "ekf_monitor<{F}, 0>"], OV, shape="lane")
    rows += _row("sia6/lane-scan-monitor", "b80", [FWD_SYM, BWD_SYM, PINV, "ekf_monitor<{F}, 21>"], OV, shape="lane", test_flags=2)
    rows += _row("sia6/lane-L50", "b80-L50", [_sym(mon=1), BWD_SYM, PINV], OV, shape="lane")
    rows += _row("sia3/lane-L5", "cfg3-L5", [FWD_SYM, BWD_SYM, PINV, "ekf_monitor<{F}, 0>"], OV, shape="lane")
    rows += _row("f32/cfg4-L50", "b80-L50", [_sym(stor=1, mon=1), "eks_bwd_sym<{M}, {F}, 1>", PINV], OV, second=[], storage="f32", shape="lane")
    rows += _row("f32/cfg3-L50", "cfg3-L50", [_sym(stor=1, mon=1), "eks_bwd_sym<{M}, {F}, 1>", PINV], OV, second=[], storage="f32", shape="lane")
    rows += _row("sia3/lane-L50", "cfg3-L50", [_sym(mon=1), BWD_SYM, PINV], OV, shape="lane")
    # the dense pair of the 3-state models (a non-diagonal Q_w)
    rows += _row("sia3/dense", "cfg3-dense", DENSE + [PINV], "", hint=2, second=[], shape="lane")
    # the second pass of exact_nonfinite with a chain to run: eks_pinv<M, 1> over the list of marked chains
    rows += _row("sia6/overflow-second-pass", "b80-overflow", [FWD_SYM, BWD_SYM, PINV, PAR], OV, shape="lane", guard=True)
    rows += _row("sia3/overflow-second-pass", "cfg3-overflow", [FWD_SYM, BWD_SYM, PINV, PAR], OV, shape="lane", guard=True)
    # the sweep entry: the smoother cut where the horizon ends, the scoring tail beside the observed days
    rows += _row("sweep/blk40-horizon", "sweep80", [FWD_SYM, L6 % (40, 1), PINV, PAR], "OVERLAP|BWD_HORIZON", flips=(0,), entry="sweep", t_hist=30,
                 shape="lane", lane_block=40)
    rows += _row("sweep/hex-reverse-pipe", "sweep80", ["ekf_fwd_hex<{F}, 10, 1>", "eks_bwd_hex<{F}, 10, 2>", PINV, PAR],
                 "OVERLAP|REVERSE_PIPE|BWD_HORIZON", flips=(0,), entry="sweep", t_hist=30, shape="hex", lane_block=10, test_flags=1)
    ids = [r["id"] for r in rows]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return rows


LEDGER = _rows()
BY_ID = {r["id"]: r for r in LEDGER}


# ---------------------------------------------------------------- a row's descriptor, as EkfRunner builds it
def planned_desc(row, w=None):
    """The epi_batch_desc of a row's call -- what batch.EkfRunner passes (its own precheck answers path_hint = row["hint"])."""
    from epidemicmodeling_amd import _lib, batch
    w = workload(row["workload"], row["flipped"]) if w is None else w
    kw = row["runner"]
    names = list(batch.OUT_NAMES) if kw["outputs"] is None else list(kw["outputs"])
    if w.model.startswith("NewCase") and "u_opt_smooth" in names:
        names.remove("u_opt_smooth")
    d = _lib.make_desc(w.model, w.B, w.T, w.Sx, w.Su, w.n_npi, w.L, w.order, w.obs_type, 1 if w.R_series is not None else 0,
                       batch.out_mask_of(names), 1 if np.ndim(w.Q) == 3 else 0)
    d.shape = {"auto": 0, "lane": 1, "quad": 2, "wave": 3, "hex": 4}[kw["shape"]]
    d.storage = {"f64": 0, "f32": 1}[kw["storage"]]
    d.test_window, d.test_flags, d.time_pipe = kw["test_window"], kw["test_flags"], kw["time_pipe"]
    blk = kw["lane_block"]
    d.lane_block = 0 if (blk <= 0 or blk >= w.B) else blk
    d.path_hint = row["hint"]
    return d


def desc_fields(d):
    return {n: int(getattr(d, n)) for n, _ in d._fields_}


def coverage_table():
    """Markdown lines 'instance | rows' over the ledger: what DESIGN.md 2 and the README quote (python -m tests.kernel_ledger)."""
    by = {}
    for r in LEDGER:
        for n in r["names"] + (r["second"] if r["guard"] else []):
            by.setdefault(n, []).append(r["id"])
    lines = ["| kernel instance | ledger rows that launch it |", "|---|---|"]
    for n in sorted(by):
        ids = by[n]
        lines.append("| `%s` | %s%s |" % (n, ", ".join(ids[:3]), " (+%d more)" % (len(ids) - 3) if len(ids) > 3 else ""))
    return lines


def readme_line():
    n = len(coverage_table()) - 2
    return ("`tests/kernel_ledger.py` names, for each of the %d launchable instances of the filter kernels (forward, smoother, monitor, "
            "dense pair, pinv grid; %d more are compiled and never launched), the test calls that run it: %d rows, each checked against the "
            "launch plan on a CPU and run against the oracle on the device." % (n, len(NEVER_LAUNCHED), len(LEDGER)))


if __name__ == "__main__":
    print("%d rows, %d instances" % (len(LEDGER), len(coverage_table()) - 2))
    print("\n".join(coverage_table()))
    print(readme_line())
