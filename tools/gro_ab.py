#!/usr/bin/env python3
"""Same-process timing of receive coalescing against the two passes around it.

    python tools/gro_ab.py [--rounds 10] [--launches 10] [--shape all|mss1460|mss1448|jumbo|single] [--ipver 0|4|6]

Shapes (each for IPv4 and IPv6, no options, frames made on the device by segmentation offload itself):
  mss1460  23,832 runs of 44 frames of 1460 B payload: 1,048,608 frames.
  mss1448  the same at 1448 B.
  jumbo    37,450 runs of 7 frames of 8960 B: 262,150 frames.
  single   1,048,576 frames of 40-100 B payload, every one its own connection: nothing coalesces.
Per shape four legs are timed in interleaved rounds whose order alternates, `--launches` back-to-back calls bracketed
by HIP events on the launch stream:
  tso   nsx_tso_*_build_dev of the mirrored batch (the same bytes moved the other way: the yardstick);
  rx    nsx_rx_*_tcp_verify_dev over the frames;
  gro   the whole nsx_gro_*_tcp_dev call (its five launches);
  tso2  the tso leg again — the difference between the two is the run-to-run spread of this process.
Before timing, gro's output is checked: n_super, frame_cnt and the payload bytes equal the batch the frames were cut
from. The time of each of gro's launches comes from a separate run of this tool under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/gro_ab.py --shape mss1460 --ipver 4); the copy kernel's rate is
(frame bytes read + payload bytes written) / its time there, the project's convention.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network-stack_amd")]


def wrap(x, bits, torch):
    """int64 tensor → the signed `bits`-wide integer holding its low bits."""
    half = 1 << (bits - 1)
    return ((x + half) % (1 << bits) - half).to({16: torch.int16, 32: torch.int32}[bits])


def shape(tag, ipver, nsup, cnt, mss, rounds, launches, ragged=False):
    import bench
    import nsx
    import torch
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
    mask = torch.empty((nf + 63) // 64, dtype=torch.int64, device=dev)
    work = torch.empty(nsx.gro_work_bytes(nf), dtype=torch.uint8, device=dev)

    def tso():
        tso_fn(ip, sup, data, sdoff, dmss, first, fseg, frames, out_off)

    def rx():
        rx_fn(frames, out_off, mask=mask)

    tso()
    rx()
    out = gro_fn(frames, out_off, mask, work=work)

    def gro():
        gro_fn(frames, out_off, mask, out=out, work=work)

    torch.cuda.synchronize()
    ns = int(out["n_super"].item())
    ok = ns == nsup and bool((out["frame_cnt"][:ns] == cnt).all()) and bool(torch.equal(out["data"][:total], data)) \
        and bool(torch.equal(out["data_off"][:ns + 1], sdoff)) and bool(torch.equal(out["seq_num"][:ns], sup["seq_num"]))
    print(f"parity {tag}: n_super {ns} of {nsup}, runs, offsets, sequence numbers and {total / 1e6:.1f} MB of payload: "
          f"{'same' if ok else 'MISMATCH'}", flush=True)
    if not ok:
        raise SystemExit("receive coalescing did not give back the batch the frames were cut from")
    moved = {"tso": total + fbytes, "tso2": total + fbytes, "rx": fbytes, "gro": fbytes + total}
    legs = [("tso", tso), ("rx", rx), ("gro", gro), ("tso2", tso)]
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
        rate = moved[name] / (med[name] * 1e-3) / 1e9
        print(f"GROAB {tag} {name:5s} median {med[name]:.5f} ms/call  min {v[0]:.5f} max {v[-1]:.5f}  moved "
              f"{moved[name] / 1e6:.1f} MB  {rate:.1f} GB/s  frac of HBM peak {rate / bench.HBM_PEAK_GBPS:.4f}", flush=True)
    spread = abs(med["tso"] - med["tso2"]) / min(med["tso"], med["tso2"])
    print(f"GROAB {tag}: frames {nf} ({fbytes / 1e6:.1f} MB), whole gro call vs tso build "
          f"{med['gro'] / min(med['tso'], med['tso2']):.4f}, vs rx {med['gro'] / med['rx']:.4f}; "
          f"spread between the two tso legs {spread * 100:.2f}%", flush=True)


SHAPES = {"mss1460": (23832, 44, 1460, False), "mss1448": (23832, 44, 1448, False), "jumbo": (37450, 7, 8960, False),
          "single": (1 << 20, 1, 100, True)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--shape", default="all", choices=["all"] + list(SHAPES))
    ap.add_argument("--ipver", type=int, default=0, choices=[0, 4, 6])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for name, (nsup, cnt, mss, ragged) in SHAPES.items():
        if a.shape not in ("all", name):
            continue
        for ipver in (4, 6):
            if a.ipver in (0, ipver):
                shape(f"{name}_v{ipver}", ipver, nsup, cnt, mss, a.rounds, a.launches, ragged)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
