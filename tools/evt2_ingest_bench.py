"""Event ingest from Prophesee EVT 2.0 / 2.1 words: the device decode against a host decode in front of the record call,
PCIe-inclusive, on one handle (GPU box).  The twin of tools/evt3_ingest_bench.py.

The source is the left camera of bench.py's DSEC workload, quantised to microseconds, sorted by (us, y, polarity, x) and encoded
as EVT 2.0 (one word per event, a TIME_HIGH word where us >> 6 changes) and as EVT 2.1 (one word per group of equal
(us, y, polarity, x >> 5), valid bit x & 31), cut into packets of a given number of events ("tick": the workload's 10 ms ticks,
~196 k events).  Every route stages the same packets into a freshly reset handle:

  a   esvo_evt2_to_events on the host (the library's decoder, into a buffer allocated once) + ts_push_events    16 B/event up
  b   ts_push_evt2 on the host words, pageable                                                                  4 or 8 B/word up, 8 B/event down
  c   ts_push_evt2 on the words in device memory (one torch tensor, uploaded before)                           8 B/event down

b and c are measured with the device decode forced for every packet (esvo_debug_evt2_device_min 0), so that the table shows
where it starts to pay; route b_default is ts_push_evt2 as shipped (small packets take the host decoder).  The routes alternate
inside every repetition; a route's time is the time inside its calls.  Median, best and worst over the repetitions.  All routes are
checked once to leave the same event ring.  No pass threshold: a measurement.

usage: python tools/evt2_ingest_bench.py [--reps N (>= 3, default 5)] [--ticks 40] [--sizes 2000,8000,16000,tick] [--formats 20,21]
                                         [--out FILE.txt]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib import workload  # noqa: E402
from esvo_amd import abi, lib  # noqa: E402

ROUTES = ("a", "b", "c", "b_default")
NAMES = {abi.EVT_2_0: "EVT 2.0", abi.EVT_2_1: "EVT 2.1", abi.EVT_2_1_LEGACY: "EVT 2.1 legacy"}
TIME_HIGH = 0x8


def encode(x, y, t_us, p, fmt):
    """the memory image (uint32) of events sorted by (t_us, y, p, x), t_us in [0, 2^34); a packet opens with TIME_HIGH, so it decodes
    alone"""
    u = np.uint64
    x, y, t, p = (np.asarray(v).astype(u) for v in (x, y, t_us, p))
    n = len(x)
    if n == 0:
        return np.zeros(0, np.uint32)
    assert int(t.max()) < 2 ** 34
    if fmt == abi.EVT_2_0:
        hi = t >> u(6)
        words = np.stack([u(TIME_HIGH << 28) | hi, p << u(28) | (t & u(63)) << u(22) | x << u(11) | y], 1)
        keep = np.ones(words.shape, bool)
        keep[1:, 0] = hi[1:] != hi[:-1]
        return words[keep].astype(np.uint32)
    first = np.ones(n, bool)   # the first event of a group: same microsecond, row, polarity and block of 32 pixels
    first[1:] = (t[1:] != t[:-1]) | (y[1:] != y[:-1]) | (p[1:] != p[:-1]) | (x[1:] >> u(5) != x[:-1] >> u(5)) | (x[1:] <= x[:-1])
    g0 = np.flatnonzero(first)
    valid = np.bitwise_or.reduceat(u(1) << (x & u(31)), g0)
    gt, hi = t[g0], t[g0] >> u(6)
    words = np.stack([u(TIME_HIGH << 60) | hi << u(32), p[g0] << u(60) | (gt & u(63)) << u(54) | (x[g0] >> u(5) << u(5)) << u(43) | y[g0] << u(32) | valid], 1)
    keep = np.ones(words.shape, bool)
    keep[1:, 0] = hi[1:] != hi[:-1]
    halves = words[keep].astype("<u8").view("<u4").reshape(-1, 2)
    return (halves if fmt == abi.EVT_2_1 else halves[:, ::-1]).reshape(-1).copy()


def packets_of(stream, ticks, size, fmt):
    """-> (t_offset_us, [(words, events)]): the left camera cut into packets of `size` events ("tick": the workload's ticks)"""
    ev = stream.ev_left
    us = (abi.event_ns(ev) // np.uint64(1000)).astype(np.int64)
    base = int(us[0]) - 1000
    t_first = ticks[0][0] - int(workload.TICK_S * 1e9)
    edges = [int(np.searchsorted(us, t // 1000, side="left")) for t in [t_first] + [tk[0] for tk in ticks]]
    if size != "tick":
        edges = list(range(edges[0], min(edges[-1], edges[0] + 200 * size), size))
    out = []
    for lo, hi in zip(edges, edges[1:]):
        if hi <= lo:
            continue
        order = np.lexsort((ev["x"][lo:hi], ev["polarity"][lo:hi] != 0, ev["y"][lo:hi], us[lo:hi])) + lo
        out.append((encode(ev["x"][order], ev["y"][order], us[order] - base, ev["polarity"][order] != 0, fmt), hi - lo))
    return base, out


def run_route(dev, route, packets, dwords, base, scratch, fmt):
    """-> (seconds inside the calls, of which in the host decoder, events); dev: the handle whose bounds the route is measured with"""
    dev.reset()
    so = lib.load()
    st, n_out = abi.Evt2State(), C.c_size_t(0)
    t_call = t_dec = 0.0
    n = at = 0
    for words, n_ev in packets:
        if route == "a":
            t0 = time.perf_counter()
            rc = so.esvo_evt2_to_events(C.byref(st), words.ctypes.data, words.nbytes, fmt, base, scratch.ctypes.data, scratch.size, C.byref(n_out), None)
            t1 = time.perf_counter()
            assert rc == 0 and n_out.value == n_ev
            dev.ts_push_events(0, scratch[:n_ev])
            t2 = time.perf_counter()
            t_dec += t1 - t0
            t_call += t2 - t0
        else:
            src = dwords[at:at + words.size] if route == "c" else words
            t0 = time.perf_counter()
            got = dev.ts_push_evt2(0, src, fmt, base)
            t_call += time.perf_counter() - t0
            assert got == n_ev
        at += words.size
        n += n_ev
    return t_call, t_dec, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--sizes", default="2000,8000,16000,tick")
    ap.add_argument("--formats", default="20,21")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.reps >= 3
    import torch
    rig, stream, p, ticks = workload.make_workload("dsec640x480", a.ticks)
    forced = lib.Esvo(p, rig)      # every packet decoded on the device
    forced.debug_evt2_device_min(0)
    shipped = lib.Esvo(p, rig)     # the bounds the library ships with
    lines = []
    for fmt in [int(f) for f in a.formats.split(",")]:
        for size in [s if s == "tick" else int(s) for s in a.sizes.split(",")]:
            base, packets = packets_of(stream, ticks, size, fmt)
            all_words = np.concatenate([w for w, _ in packets])
            dwords = torch.from_numpy(all_words.view(np.int32)).cuda()
            torch.cuda.synchronize()
            scratch = np.zeros(max(n for _, n in packets), abi.EVENT_DTYPE)

            def run(r):
                return run_route(shipped if r == "b_default" else forced, r, packets, dwords, base, scratch, fmt)

            tails = {}
            for r in ROUTES:   # every route leaves the same ring
                _, _, n = run(r)
                k = min(n, 4096)
                ev, stamps, b0, b1 = (shipped if r == "b_default" else forced).debug_ts_ring(0, n - k, k)
                tails[r] = (ev.tobytes(), stamps.tobytes(), b0, b1)
            assert all(tails[r] == tails["a"] for r in ROUTES), "the routes leave different event rings"
            res = {r: dict(call=[], dec=[]) for r in ROUTES}
            for rep in range(a.warmup + a.reps):
                for r in ROUTES[rep % len(ROUTES):] + ROUTES[:rep % len(ROUTES)]:
                    t_call, t_dec, n = run(r)
                    if rep >= a.warmup:
                        res[r]["call"].append(t_call * 1e3 / len(packets))
                        res[r]["dec"].append(t_dec * 1e3 / len(packets))
            n_ev = n // len(packets)
            n_words = all_words.size // (1 if fmt == abi.EVT_2_0 else 2)
            line = {"bench": "evt2_ingest", "format": NAMES[fmt], "workload": "dsec640x480", "camera": "left", "packet": size, "packets": len(packets),
                    "events_per_packet": int(n_ev), "words_per_event": round(n_words / n, 3), "bytes_per_packet": int(all_words.nbytes // len(packets)),
                    "reps": a.reps, "routes": {}}
            for r in ROUTES:
                v = np.asarray(res[r]["call"])
                line["routes"][r] = {"ms_per_call_median": round(float(np.median(v)), 4), "ms_per_call_best": round(float(v.min()), 4),
                                     "ms_per_call_worst": round(float(v.max()), 4), "events_per_s_median": round(n_ev / float(np.median(v)) * 1e3),
                                     "host_decode_ms_median": round(float(np.median(res[r]["dec"])), 4)}
            print(json.dumps(line), flush=True)
            lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("# tools/evt2_ingest_bench.py: ms per call, median (best - worst) over %d alternating repetitions; M events/s at the median\n" % a.reps)
            f.write("# a: host decode + ts_push_events (of which host decode); b / c: ts_push_evt2, host / device words, device decode forced;\n")
            f.write("# b_default: ts_push_evt2 on host words as shipped\n")
            f.write("%-8s %10s %8s %6s %9s | %s\n" % ("format", "ev/packet", "packets", "w/ev", "B/packet", " | ".join("%-34s" % r for r in ROUTES)))
            for ln in lines:
                cells = []
                for r in ROUTES:
                    q = ln["routes"][r]
                    cell = "%.4f (%.4f - %.4f) %6.1f M" % (q["ms_per_call_median"], q["ms_per_call_best"], q["ms_per_call_worst"], q["events_per_s_median"] / 1e6)
                    cells.append("%-34s" % (cell + (" [dec %.4f]" % q["host_decode_ms_median"] if r == "a" else "")))
                f.write("%-8s %10d %8d %6.3f %9d | %s\n" % (ln["format"], ln["events_per_packet"], ln["packets"], ln["words_per_event"], ln["bytes_per_packet"], " | ".join(cells)))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    forced.close(); shipped.close()


if __name__ == "__main__":
    main()
