#!/usr/bin/env python3
"""Same-process timing of flow-keyed receive coalescing (nsx_gro_flow_*) against coalescing by adjacency (nsx_gro_*).

    python tools/gro_flow_ab.py [--rounds 10] [--launches 10] [--shape all|mss1460|single] [--ipver 0|4|6]
                                [--legs gro,flow_grouped,flow_inter,gro2] [--rows 0]

Shapes (each for IPv4 and IPv6, no options, frames made on the device by segmentation offload itself, as
tools/gro_ab.py makes them):
  mss1460  23,832 runs of 44 frames of 1460 B payload: 1,048,608 frames.
  single   1,048,576 frames of 40-100 B payload, every one its own connection: nothing coalesces.
Each shape once grouped (a run's frames back to back, as the offload cuts them) and once interleaved: the runs taken
64 at a time and delivered round-robin, frame j of each of the 64 connections, then frame j + 1 of each — what a
receive queue fed by RSS looks like. (For `single` a run is one frame, so the interleaved batch is the grouped one.)
Per shape four legs are timed in interleaved rounds whose order alternates, `--launches` back-to-back calls bracketed
by HIP events on the launch stream:
  gro           nsx_gro_*_tcp_dev over the grouped frames (the parent's call: the yardstick);
  flow_grouped  nsx_gro_flow_*_tcp_dev over the same grouped frames: the difference to gro is what the key pass, the
                sort and the index indirection cost when there was nothing to gain;
  flow_inter    nsx_gro_flow_*_tcp_dev over the interleaved frames;
  gro2          the gro leg again — the difference between the two is the run-to-run spread of this process.
Before timing, the interleaved run is checked against the batch the frames were cut from: n_super, every run's
length, and every super-segment's payload bytes (found through first_frame, d_order and the interleave). The time of
each launch comes from a separate run under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/gro_flow_ab.py --shape mss1460 --ipver 4 --legs gro,flow_inter);
a copy kernel's rate is (frame bytes read + payload bytes written) / its time there, the project's convention.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network-stack_amd"), os.path.join(ROOT, "tools")]

LEGS = ("gro", "flow_grouped", "flow_inter", "gro2")
CONNS = 64


def interleave(nsup, cnt, torch, dev):
    """perm[p] = the grouped frame delivered at position p: the runs 64 at a time, round-robin inside each set."""
    parts = []
    for r0, runs in ((0, nsup - nsup % CONNS), (nsup - nsup % CONNS, nsup % CONNS)):
        if runs == 0:
            continue
        per = min(runs, CONNS)
        run = r0 + torch.arange(runs, dtype=torch.int64, device=dev).view(-1, 1, per)      # set, (frame), connection
        j = torch.arange(cnt, dtype=torch.int64, device=dev).view(1, cnt, 1)
        parts.append((run * cnt + j).reshape(-1))
    return torch.cat(parts)


def shape(tag, ipver, nsup, cnt, mss, rounds, launches, ragged, legs, tune):
    import bench
    import nsx
    import torch
    from gro_ab import wrap
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0x770 + mss + ipver)
    ri = lambda hi, n, dt: torch.randint(0, hi, (n,), generator=g, device=dev, dtype=torch.int64).to(dt)  # noqa: E731
    iph, alen = (20, 4) if ipver == 4 else (40, 16)
    if ragged:  # one frame per super-segment, 40-100 B of payload in multiples of 4
        lens = 4 * torch.randint(10, 26, (nsup,), generator=g, device=dev, dtype=torch.int64)
    else:
        lens = torch.full((nsup,), cnt * mss, dtype=torch.int64, device=dev)
    nf = nsup * cnt
    sup = {"src_port": ri(1 << 16, nsup, torch.int16), "dst_port": ri(1 << 16, nsup, torch.int16),
           "seq_num": wrap(ri(1 << 32, nsup, torch.int64), 32, torch),
           "ack_num": wrap(ri(1 << 32, nsup, torch.int64), 32, torch),
           "offset": torch.full((nsup,), 0x50, dtype=torch.uint8, device=dev),  # data offset 5, as on the wire
           "control": torch.full((nsup,), 0x10, dtype=torch.uint8, device=dev),
           "window": ri(1 << 16, nsup, torch.int16), "urgent_ptr": ri(1 << 16, nsup, torch.int16)}
    ip = {"src": ri(256, alen * nsup, torch.uint8), "dst": ri(256, alen * nsup, torch.uint8),
          "ident": ri(1 << 16, nsup, torch.int16), "ttl": ri(256, nsup, torch.uint8),
          "tclass": ri(256, nsup, torch.uint8), "flow": ri(1 << 20, nsup, torch.int32)}
    sdoff = torch.zeros(nsup + 1, dtype=torch.int64, device=dev)
    sdoff[1:] = torch.cumsum(lens, 0)
    total = int(sdoff[-1].item())
    data = torch.empty(total, dtype=torch.uint8, device=dev)
    nsx.fill_splitmix64_dev(data, 0x770)
    dmss = torch.full((nsup,), mss, dtype=torch.int32, device=dev)
    first = torch.arange(nsup + 1, dtype=torch.int64, device=dev) * cnt
    fseg = (torch.arange(nf, dtype=torch.int64, device=dev) // cnt).to(torch.int32)
    flen = (lens + iph + 20) if ragged else torch.full((nf,), mss + iph + 20, dtype=torch.int64, device=dev)
    out_off = torch.zeros(nf + 1, dtype=torch.int64, device=dev)
    out_off[1:] = torch.cumsum(flen, 0)  # every frame a multiple of 4 bytes: the build's slots are rx's offsets
    fbytes = int(out_off[-1].item())
    frames = torch.empty(fbytes, dtype=torch.uint8, device=dev)
    tso_fn = nsx.tso_ipv4_tcp_build_dev if ipver == 4 else nsx.tso_ipv6_tcp_build_dev
    rx_fn = nsx.rx_ipv4_tcp_verify_dev if ipver == 4 else nsx.rx_ipv6_tcp_verify_dev
    gro_fn = nsx.gro_ipv4_tcp_dev if ipver == 4 else nsx.gro_ipv6_tcp_dev
    flow_fn = nsx.gro_flow_ipv4_tcp_dev if ipver == 4 else nsx.gro_flow_ipv6_tcp_dev
    tso_fn(ip, sup, data, sdoff, dmss, first, fseg, frames, out_off)
    mask = rx_fn(frames, out_off)  # all ones here, so it serves the interleaved frames as well
    if cnt > 1:  # equal frame lengths: the interleaved batch is a row gather, its offsets the same
        perm = interleave(nsup, cnt, torch, dev)
        inter = frames.view(nf, mss + iph + 20)[perm].reshape(-1).contiguous()
    else:
        perm = torch.arange(nf, dtype=torch.int64, device=dev)
        inter = frames
    work = torch.empty(nsx.gro_flow_work_bytes(nf), dtype=torch.uint8, device=dev)
    order = torch.empty(nf, dtype=torch.int32, device=dev)
    out = gro_fn(frames, out_off, mask, work=work)

    steps = {"gro": lambda: gro_fn(frames, out_off, mask, out=out, work=work),
             "flow_grouped": lambda: flow_fn(frames, out_off, mask, out=out, order=order, work=work, tune=tune),
             "flow_inter": lambda: flow_fn(inter, out_off, mask, out=out, order=order, work=work, tune=tune)}
    steps["gro2"] = steps["gro"]

    # parity of the interleaved run: super-segment s is run (perm[order[first_frame[s]]] // cnt) of the batch
    steps["flow_inter"]()
    torch.cuda.synchronize()
    ns = int(out["n_super"].item())
    ok = ns == nsup and bool((out["frame_cnt"][:ns] == cnt).all()) and int(out["data_off"][ns].item()) == total
    if ok:
        run = perm[order.to(torch.int64)[out["first_frame"][:ns]]] // cnt
        ok = bool(torch.equal(torch.sort(run).values, torch.arange(nsup, dtype=torch.int64, device=dev)))
        ok = ok and bool(torch.equal(out["seq_num"][:ns], sup["seq_num"][run]))
        ok = ok and bool(torch.equal(out["data_off"][1:ns + 1] - out["data_off"][:ns], lens[run]))
        if ragged:
            seg = torch.repeat_interleave(torch.arange(ns, dtype=torch.int64, device=dev), lens[run])
            src = sdoff[run][seg] + torch.arange(total, dtype=torch.int64, device=dev) - out["data_off"][:ns][seg]
            ok = ok and bool(torch.equal(out["data"][:total], data[src]))
            del seg, src
        else:
            ok = ok and bool(torch.equal(out["data"][:total].view(nsup, cnt * mss), data.view(nsup, cnt * mss)[run]))
    print(f"parity {tag} interleaved: n_super {ns} of {nsup}, run lengths, sequence numbers and "
          f"{total / 1e6:.1f} MB of payload per super-segment: {'same' if ok else 'MISMATCH'}", flush=True)
    if not ok:
        raise SystemExit("flow-keyed coalescing did not give back the batch the frames were cut from")
    torch.cuda.empty_cache()
    moved = fbytes + total
    legs = [(name, steps[name]) for name in LEGS if name in legs]
    t_end = time.perf_counter() + 0.5
    while time.perf_counter() < t_end:  # settle
        for _, step in legs:
            step()
        torch.cuda.synchronize()
    res = {name: [] for name, _ in legs}
    for r in range(rounds):
        for name, step in (legs if r % 2 == 0 else legs[::-1]):
            for _ in range(2):
                step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                step()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / launches)
    med = {k: statistics.median(v) for k, v in res.items()}
    for name, v in res.items():
        v = sorted(v)
        rate = moved / (med[name] * 1e-3) / 1e9
        print(f"GROFLOWAB {tag} {name:12s} median {med[name]:.5f} ms/call  min {v[0]:.5f} max {v[-1]:.5f}  moved "
              f"{moved / 1e6:.1f} MB  {rate:.1f} GB/s  frac of HBM peak {rate / bench.HBM_PEAK_GBPS:.4f}", flush=True)
    if all(k in med for k in LEGS):
        base = min(med["gro"], med["gro2"])
        spread = abs(med["gro"] - med["gro2"]) / base
        print(f"GROFLOWAB {tag}: frames {nf} ({fbytes / 1e6:.1f} MB); key pass + sort + indirection over grouped "
              f"frames {med['flow_grouped'] - base:+.5f} ms ({med['flow_grouped'] / base:.4f} of gro), interleaved "
              f"{med['flow_inter'] / base:.4f} of gro; spread between the two gro legs {spread * 100:.2f}%", flush=True)


SHAPES = {"mss1460": (23832, 44, 1460, False), "single": (1 << 20, 1, 100, True)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--shape", default="all", choices=["all"] + list(SHAPES))
    ap.add_argument("--ipver", type=int, default=0, choices=[0, 4, 6])
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--rows", type=int, default=0, help="keys per sort tile in units of 256 (0 = the default)")
    a = ap.parse_args()
    legs = a.legs.split(",")
    if not legs or set(legs) - set(LEGS):
        ap.error(f"--legs takes a comma-separated subset of {LEGS}")
    torch.cuda.set_device(0)
    for name, (nsup, cnt, mss, ragged) in SHAPES.items():
        if a.shape not in ("all", name):
            continue
        for ipver in (4, 6):
            if a.ipver in (0, ipver):
                shape(f"{name}_v{ipver}", ipver, nsup, cnt, mss, a.rounds, a.launches, ragged, legs,
                      dict(rows=a.rows) if a.rows else None)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
