"""Event ingest from Prophesee EVT 3.0 words: the device decode against a host decode in front of the record call, PCIe-inclusive, on
one handle (GPU box).

The source is the left camera of bench.py's DSEC workload, quantised to microseconds and encoded as EVT 3.0 (TIME_HIGH / TIME_LOW /
ADDR_Y where they change; events of one microsecond, row and polarity inside one 12-pixel window as VECT_BASE_X + VECT_12 / VECT_8,
the others as ADDR_X), cut into packets of a given number of events ("tick": the workload's 10 ms ticks, ~196 k events).  Every
route stages the same packets into a freshly reset handle:

  a   esvo_evt3_to_events on the host (the library's decoder, into a buffer allocated once) + ts_push_events    16 B/event up
  b   ts_push_evt3 on the host words, pageable                                                                  2 B/word up, 8 B/event down
  c   ts_push_evt3 on the words in device memory (one torch tensor, uploaded before)                           8 B/event down

b and c are measured with the device decode forced for every packet (esvo_debug_evt3_device_min 0), so that the table shows
where it starts to pay; route b_default is ts_push_evt3 as shipped (small packets take the host decoder).  The routes alternate
inside every repetition; a route's time is the time inside its calls.  Median, best and worst over the repetitions.  All routes are
checked once to leave the same event ring.  No pass threshold: a measurement.

usage: python tools/evt3_ingest_bench.py [--reps N (>= 3, default 5)] [--ticks 40] [--sizes 500,2000,...,tick] [--out FILE.txt]"""
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
DEFAULT_MIN = 0
TH, TL, AY, AX, VB, V12, V8 = 0x8000, 0x6000, 0x0000, 0x2000, 0x3000, 0x4000, 0x5000


def encode(x, y, t_us, p):
    """EVT 3.0 words of events sorted by (t_us, y, p, x), t_us in [0, 2^24); a packet opens with TIME_HIGH, TIME_LOW and ADDR_Y, so it
    decodes alone.  -> uint16 words"""
    x, y, t, p = (np.asarray(v).astype(np.int64) for v in (x, y, t_us, p))
    n = len(x)
    if n == 0:
        return np.zeros(0, np.uint16)
    assert t.min() >= 0 and t.max() < 2 ** 24
    first = np.ones(n, bool)   # the first event of a group: same microsecond, row, polarity and 12-pixel window, x ascending
    first[1:] = (t[1:] != t[:-1]) | (y[1:] != y[:-1]) | (p[1:] != p[:-1]) | (x[1:] // 12 != x[:-1] // 12) | (x[1:] <= x[:-1])
    g0 = np.flatnonzero(first)
    size = np.diff(np.append(g0, n))
    x0, gt, gy, gp = x[g0], t[g0], y[g0], p[g0]
    mask = np.bitwise_or.reduceat(np.int64(1) << (x - np.repeat(x0, size)), g0)
    vect = size > 1
    hi, lo = gt >> 12, gt & 0xFFF
    words = np.stack([TH | hi, TL | lo, AY | gy, np.where(vect, VB | gp << 11 | x0, 0),
                      np.where(vect, np.where(mask < 256, V8 | mask, V12 | mask), AX | gp << 11 | x0)], 1)
    keep = np.ones(words.shape, bool)
    keep[1:, 0] = hi[1:] != hi[:-1]
    keep[1:, 1] = gt[1:] != gt[:-1]
    keep[1:, 2] = gy[1:] != gy[:-1]
    keep[:, 3] = vect
    return words[keep].astype(np.uint16)


def packets_of(stream, ticks, size):
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
        out.append((encode(ev["x"][order], ev["y"][order], us[order] - base, ev["polarity"][order] != 0), hi - lo))
    return base, out


def run_route(dev, route, packets, dwords, base, scratch):
    """-> (seconds inside the calls, of which in the host decoder, events)"""
    dev.reset()
    dev.debug_evt3_device_min(DEFAULT_MIN if route == "b_default" else 0)
    so = lib.load()
    st, n_out = abi.Evt3State(), C.c_size_t(0)
    t_call = t_dec = 0.0
    n = at = 0
    for words, n_ev in packets:
        if route == "a":
            t0 = time.perf_counter()
            rc = so.esvo_evt3_to_events(C.byref(st), words.ctypes.data, words.size, base, scratch.ctypes.data, scratch.size, C.byref(n_out), None)
            t1 = time.perf_counter()
            assert rc == 0 and n_out.value == n_ev
            dev.ts_push_events(0, scratch[:n_ev])
            t2 = time.perf_counter()
            t_dec += t1 - t0
            t_call += t2 - t0
        else:
            src = dwords[at:at + words.size] if route == "c" else words
            t0 = time.perf_counter()
            got = dev.ts_push_evt3(0, src, base)
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
    ap.add_argument("--sizes", default="500,1000,2000,4000,8000,16000,50000,tick")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.reps >= 3
    import torch
    rig, stream, p, ticks = workload.make_workload("dsec640x480", a.ticks)
    dev = lib.Esvo(p, rig)
    global DEFAULT_MIN
    DEFAULT_MIN = dev.debug_evt3_device_min(0)   # the bound the library ships with
    lines = []
    for size in [s if s == "tick" else int(s) for s in a.sizes.split(",")]:
        base, packets = packets_of(stream, ticks, size)
        all_words = np.concatenate([w for w, _ in packets])
        dwords = torch.from_numpy(all_words.view(np.int16)).cuda()
        torch.cuda.synchronize()
        scratch = np.zeros(max(n for _, n in packets), abi.EVENT_DTYPE)
        tails = {}
        for r in ROUTES:   # every route leaves the same ring
            _, _, n = run_route(dev, r, packets, dwords, base, scratch)
            k = min(n, 4096)
            ev, stamps, b0, b1 = dev.debug_ts_ring(0, n - k, k)
            tails[r] = (ev.tobytes(), stamps.tobytes(), b0, b1)
        assert all(tails[r] == tails["a"] for r in ROUTES), "the routes leave different event rings"
        res = {r: dict(call=[], dec=[]) for r in ROUTES}
        for rep in range(a.warmup + a.reps):
            for r in ROUTES[rep % len(ROUTES):] + ROUTES[:rep % len(ROUTES)]:
                t_call, t_dec, n = run_route(dev, r, packets, dwords, base, scratch)
                if rep >= a.warmup:
                    res[r]["call"].append(t_call * 1e3 / len(packets))
                    res[r]["dec"].append(t_dec * 1e3 / len(packets))
        n_ev = n // len(packets)
        line = {"bench": "evt3_ingest", "workload": "dsec640x480", "camera": "left", "packet": size, "packets": len(packets),
                "events_per_packet": int(n_ev), "words_per_event": round(all_words.size / n, 3), "reps": a.reps, "routes": {}}
        for r in ROUTES:
            v = np.asarray(res[r]["call"])
            line["routes"][r] = {"ms_per_call_median": round(float(np.median(v)), 4), "ms_per_call_best": round(float(v.min()), 4),
                                 "ms_per_call_worst": round(float(v.max()), 4), "events_per_s_median": round(n_ev / float(np.median(v)) * 1e3),
                                 "host_decode_ms_median": round(float(np.median(res[r]["dec"])), 4)}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("# tools/evt3_ingest_bench.py: ms per call, median (best - worst) over %d alternating repetitions; M events/s at the median\n" % a.reps)
            f.write("# a: host decode + ts_push_events (of which host decode); b / c: ts_push_evt3, host / device words, device decode forced;\n")
            f.write("# b_default: ts_push_evt3 on host words as shipped\n")
            f.write("%10s %8s %6s | %s\n" % ("ev/packet", "packets", "w/ev", " | ".join("%-34s" % r for r in ROUTES)))
            for ln in lines:
                cells = []
                for r in ROUTES:
                    q = ln["routes"][r]
                    cell = "%.4f (%.4f - %.4f) %6.1f M" % (q["ms_per_call_median"], q["ms_per_call_best"], q["ms_per_call_worst"], q["events_per_s_median"] / 1e6)
                    cells.append("%-34s" % (cell + (" [dec %.4f]" % q["host_decode_ms_median"] if r == "a" else "")))
                f.write("%10d %8d %6.3f | %s\n" % (ln["events_per_packet"], ln["packets"], ln["words_per_event"], " | ".join(cells)))
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    dev.close()


if __name__ == "__main__":
    main()
