"""Helpers of tests/test_hip_stream_order.py: every entry point behind a busy stream and on a side stream ("Stream order").

The method. A case has two valid inputs of the same shapes, A (stale) and B (fresh), and a list of `steps` (the calls under test).
  1. plain runs on the idle default stream, as every other test of the suite calls the library: out_B = op(B), then out_A = op(A) - which also leaves every
     buffer the library reads (holder tensors, snapshot, bound camera, batch buffers) holding A;
  2. on a side stream the same un-stalled run of A once more (the stream's allocator pool and the library's first-call buffers exist afterwards);
  3. the stalled run: a stall of fixed length is enqueued on the stream, then `x.copy_(B)` for every device input IN STREAM ORDER, then the steps, then
     clones of the outputs; only then the host waits and compares with out_B.
Whatever the library enqueues on another stream, and whatever the host copies too early, runs while the stall still holds the stream: it sees A, or is
overwritten by the later copy, and the result is not out_B. A is valid, so a violation is a wrong answer and never a fault.

A case passes vacuously when A and B give the same answer or when the stall has drained before the call returns; both are asserted (`assert_far_apart`,
"not exercised")."""
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

MODES = ("default_stream", "side_stream", "two_side_streams")  # (b), (c), (d) of DESIGN.md
MAX_STALL_MS = 250.0
GRAD_TOL = 1e-5  # two launches whose float atomics arrive in another order, relative to each tensor's maximum (the suite's bar)
ASYNC, SYNC, EITHER = "returns_with_the_stall_pending", "synchronises_by_design", "not_promised"

_streams = []
_cycles_per_ms = [None]


def side_streams():
    """The two side streams of the module (with the default stream: three alive at most), made on first use."""
    if not _streams:
        _streams.extend([torch.cuda.Stream(), torch.cuda.Stream()])
    return _streams


def streams_of(mode):
    if mode == "default_stream":
        return [torch.cuda.default_stream()]
    if mode == "side_stream":
        return side_streams()[:1]
    assert mode == "two_side_streams", mode
    return list(side_streams())


def _spin(cycles):
    torch.cuda._sleep(int(cycles))


def _matmul_chain(units):
    a = _matmul_chain.a
    for _ in range(int(units)):
        a = a @ _matmul_chain.a
    _matmul_chain.keep = a


def calibrate():
    """Stall units (cycles of torch.cuda._sleep; 512x512 matmuls without it) per millisecond, measured once with two events around a short stall."""
    if _cycles_per_ms[0] is not None:
        return _cycles_per_ms[0]
    if hasattr(torch.cuda, "_sleep"):
        fn, probe = _spin, 2_000_000
    else:
        _matmul_chain.a = torch.eye(512, device="cuda")
        fn, probe = _matmul_chain, 200
    fn(probe // 10)  # warm-up: the first launch of the kernel loads its code
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(probe)
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    assert ms > 0.05, ms
    _cycles_per_ms[0] = (fn, probe / ms)
    print(f"REPORT stream_order_calibration: units_per_ms={probe / ms:.0f} probe_ms={ms:.2f} stall={'_sleep' if fn is _spin else 'matmul chain'}", flush=True)
    return _cycles_per_ms[0]


def stall_ms_for(host_ms):
    """Ten times the host-side time of the plain run plus 5 ms, capped: a starting point only - that the stall is still pending is asserted."""
    return min(10.0 * host_ms + 5.0, MAX_STALL_MS)


def enqueue_stall(ms, stream):
    """A stall of about `ms` on `stream` and the event recorded right behind it: `not ev.query()` = the stall is still pending."""
    assert 0 < ms <= MAX_STALL_MS, ms
    fn, per_ms = calibrate()
    with torch.cuda.stream(stream):
        fn(per_ms * ms)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def run_steps(steps, streams, after=None):
    """The steps in host order, dealt over `streams` in turn, each stream waiting (on the device) for the one before. `after`: the stream that holds what was
    enqueued before the steps (the stall and the copies of the inputs); with two streams the first step then goes to the OTHER one. Returns the last stream."""
    prev = after
    first = 1 if after is not None and len(streams) > 1 else 0
    for k, step in enumerate(steps):
        s = streams[(k + first) % len(streams)]
        if prev is not None and s is not prev:
            s.wait_stream(prev)
        with torch.cuda.stream(s):
            step()
        prev = s
    return prev


def to_host(out):
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def bits_differ(a, b):
    """Number of elements whose bits differ, and the number compared; arrays of other shapes differ everywhere."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return max(a.size, b.size, 1), max(a.size, b.size, 1)
    w = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return int(np.count_nonzero(np.ascontiguousarray(a).view(w) != np.ascontiguousarray(b).view(w))), int(a.size)


def rel_gap(a, b):
    """max |a - b| over max |b| (the bar of two launches whose float atomics arrive in another order is relative to each tensor's maximum)."""
    scale = float(np.abs(b.astype(np.float64)).max())
    assert scale > 0.0
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) / scale


def assert_far_apart(name, out_a, out_b, tol, sizes_differ=False):
    """A and B must be far apart, or a library that read the stale input would pass: bit-equal cases differ in >= 10 % of all elements, cases with a
    tolerance by >= 100 x the tolerance in every tensor, data-dependent sizes differ too."""
    assert set(out_a) == set(out_b)
    if sizes_differ:
        assert any(out_a[k].shape != out_b[k].shape for k in out_a), (name, {k: out_a[k].shape for k in out_a})
    if tol is None:
        pairs = [bits_differ(out_a[k], out_b[k]) for k in sorted(out_a)]
        frac = sum(d for d, _ in pairs) / max(1, sum(n for _, n in pairs))
        print(f"REPORT stream_order_gap {name}: differing_elements={frac:.3f}", flush=True)
        assert frac >= 0.10, (name, frac, dict(zip(sorted(out_a), pairs)))
        return frac
    gaps = {k: rel_gap(out_a[k], out_b[k]) for k in out_a}
    print(f"REPORT stream_order_gap {name}: smallest_relative_gap={min(gaps.values()):.2e} tolerance={tol:.0e}", flush=True)
    assert min(gaps.values()) >= 100.0 * tol, (name, gaps)
    return min(gaps.values())


def assert_same(name, got, want, tol):
    assert set(got) == set(want), (name, sorted(got), sorted(want))
    for k in sorted(want):
        if tol is None:
            d, n = bits_differ(got[k], want[k])
            assert d == 0, f"{name}: '{k}' differs from the plain run of the fresh input in {d} of {n} elements (shape {got[k].shape} vs {want[k].shape})"
        else:
            assert got[k].shape == want[k].shape, (name, k)
            e = rel_gap(got[k], want[k])
            assert e <= tol, f"{name}: '{k}' is {e:.2e} of its maximum from the plain run of the fresh input (bar {tol:.0e})"


class Case:
    """What the runner needs of a case. Subclasses (or instances built with keyword arguments) provide:
      load(which)     enqueue, on the CURRENT stream and without a host wait, the copies that make every device input hold A or B (device to device, from
                      tensors made beforehand) and build fresh host arguments for `which`;
      steps()         the calls under test, one callable per call (mode (d) deals them over two streams);
      outputs()       dict name -> device tensor (the runner clones nothing itself: return clones, enqueued on the current stream);
      scribble()      after the steps, while the stall is pending: overwrite in place every host object the calls were given, and enqueue the legal writes
                      to device buffers the calls read (stream-ordered behind them).
    kind: ASYNC (hard assert: the stall is pending when the last step returns), SYNC (pending at entry), EITHER (pending at entry; reported).
    tol: None = bit equality, else the relative bar of the op's own tests. sizes_differ: the output sizes depend on the data."""
    name, kind, tol, sizes_differ = "case", EITHER, None, False

    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def scribble(self):
        pass


def run_case(case, mode):
    """Steps 1-3 of the module docstring. Returns the figures it measured."""
    name = f"{case.name}[{mode}]"
    dflt = torch.cuda.default_stream()
    plain, host_ms = {}, 0.0
    for which in ("B", "A"):  # A last: the library's own buffers hold the stale state afterwards
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        case.load(which)
        run_steps(case.steps(), [dflt])
        host_ms = 1e3 * (time.perf_counter() - t0)  # (the second run's: the first one may allocate)
        out = case.outputs()
        torch.cuda.synchronize()
        plain[which] = to_host(out)
    gap = assert_far_apart(name, plain["A"], plain["B"], case.tol, case.sizes_differ)
    streams = streams_of(mode)
    if mode != "default_stream":  # the un-stalled run on the side stream(s): A again
        with torch.cuda.stream(streams[0]):
            case.load("A")
        last = run_steps(case.steps(), streams, after=streams[0])
        with torch.cuda.stream(last):
            out = case.outputs()
        torch.cuda.synchronize()
        assert_same(name + " un-stalled", to_host(out), plain["A"], case.tol)
    torch.cuda.synchronize()
    stall_ms = stall_ms_for(host_ms)
    ev = enqueue_stall(stall_ms, streams[0])
    with torch.cuda.stream(streams[0]):
        case.load("B")
    pending_at_entry = not ev.query()
    last = run_steps(case.steps(), streams, after=streams[0])
    pending_at_return = not ev.query()
    with torch.cuda.stream(last):
        case.scribble()
        out = case.outputs()
    still_pending = not ev.query()
    last.synchronize()
    torch.cuda.synchronize()
    print(f"REPORT stream_order {name}: kind={case.kind} host_ms={host_ms:.2f} stall_ms={stall_ms:.1f} pending_at_entry={pending_at_entry} "
          f"pending_at_return={pending_at_return} pending_after_scribble={still_pending}", flush=True)
    assert pending_at_entry, f"{name}: not exercised - the stall of {stall_ms:.0f} ms had drained before the call"
    if case.kind == ASYNC:
        assert pending_at_return, f"{name}: not exercised - the stall of {stall_ms:.0f} ms was no longer pending when the call returned (it blocks, or the stall is too short)"
    assert_same(name, to_host(out), plain["B"], case.tol)
    return dict(host_ms=host_ms, stall_ms=stall_ms, gap=gap, pending_at_return=pending_at_return)


class DeviceInputs:
    """Persistent device buffers with an A and a B value each: `load(which)` is one device-to-device copy per buffer on the current stream."""

    def __init__(self, a, b):
        assert set(a) == set(b)
        self.store = {"A": {k: v.clone() for k, v in a.items()}, "B": {k: v.clone() for k, v in b.items()}}
        for k in a:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].is_cuda and b[k].is_cuda, k
        self.buf = {k: v.clone() for k, v in a.items()}

    def load(self, which):
        for k, t in self.buf.items():
            t.copy_(self.store[which][k])

    def __getitem__(self, k):
        return self.buf[k]
