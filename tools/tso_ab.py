#!/usr/bin/env python3
"""Same-process A/B of segmentation offload against the per-frame transmit pass it spares the caller.

    python tools/tso_ab.py [--rounds 20] [--launches 20] [--shape all|dev|jumbo|host]

Three shapes, IPv4, no options:
  dev    23,302 super-segments of 65,700 B (45 x 1460) at MSS 1460: 1,048,590 frames, workload 6's frame shape.
  jumbo  37,450 super-segments of 62,720 B (7 x 8960) at MSS 8960: 262,150 frames, workload 12's frame shape.
  host   2,048 of the dev shape's super-segments from host memory, pinned and pageable (--host-n overrides).
Per shape:
  (a) the parent's capability: nsx_tx_ipv4_tcp_build_dev / _host over the pre-expanded per-frame arrays (every field
      repeated per frame, seq / control / ident per the rules of nsx_csum.h, the cut points as data_off), already
      resident where the call wants them;
  (b) nsx_tso_ipv4_tcp_build_dev / _host over the super-segment arrays and the frame map.
(b)'s frames and raw sums are first checked equal to (a)'s. Then both are timed in interleaved rounds whose order
alternates: device shapes as `--launches` back-to-back calls bracketed by HIP events on the launch stream, host shapes
as wall time per call. Prints per variant the median per call, its spread over the rounds, the bytes moved (device:
read + written by the kernel; host: H2D bytes) and the rate. The margin for any comparison is (a)'s own spread in this
process.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network-stack_amd")]

TCP_B, IP4_B = 18, 11  # bytes of TCP fields / of IPv4 fields (src, dst, ident, ttl) per array entry


def report(tag, res, moved, what):
    import bench
    for name, v in res.items():
        v = sorted(v)
        med = statistics.median(v)
        q1, q3 = v[len(v) // 4], v[(3 * len(v)) // 4]
        rate = moved[name] / (med * 1e-3) / 1e9
        peak = f"  frac of HBM peak {rate / bench.HBM_PEAK_GBPS:.4f}" if what == "moved" else ""
        print(f"TSOAB {tag} {name:12s} median {med:.5f} ms/call  min {v[0]:.5f} max {v[-1]:.5f} iqr {q3 - q1:.5f} "
              f"spread {(v[-1] - v[0]) / med * 100:.2f}%  {what} {moved[name] / 1e6:.1f} MB  {rate:.1f} GB/s{peak}",
              flush=True)


def wrap(x, bits, torch):
    """int64 tensor → the signed `bits`-wide integer holding its low bits."""
    half = 1 << (bits - 1)
    return ((x + half) % (1 << bits) - half).to({16: torch.int16, 32: torch.int32}[bits])


def device_shape(tag, nsup, cnt, mss, rounds, launches):
    import nsx
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0x750 + mss)
    ri = lambda hi, n, dt: torch.randint(0, hi, (n,), generator=g, device=dev, dtype=torch.int64).to(dt)  # noqa: E731
    L, nf = cnt * mss, nsup * cnt
    sup = {"src_port": ri(1 << 16, nsup, torch.int16), "dst_port": ri(1 << 16, nsup, torch.int16),
           "seq_num": wrap(ri(1 << 32, nsup, torch.int64), 32, torch), "ack_num": wrap(ri(1 << 32, nsup, torch.int64), 32, torch),
           "offset": torch.full((nsup,), 5, dtype=torch.uint8, device=dev), "control": ri(256, nsup, torch.uint8),
           "window": ri(1 << 16, nsup, torch.int16), "urgent_ptr": ri(1 << 16, nsup, torch.int16)}
    ip = {"src": ri(256, 4 * nsup, torch.uint8), "dst": ri(256, 4 * nsup, torch.uint8),
          "ident": ri(1 << 16, nsup, torch.int16), "ttl": ri(256, nsup, torch.uint8)}
    data = torch.empty(nsup * L, dtype=torch.uint8, device=dev)
    nsx.fill_splitmix64_dev(data, 0x750)
    sdoff = torch.arange(nsup + 1, dtype=torch.int64, device=dev) * L
    dmss = torch.full((nsup,), mss, dtype=torch.int32, device=dev)
    first = torch.arange(nsup + 1, dtype=torch.int64, device=dev) * cnt
    seg = torch.arange(nf, dtype=torch.int64, device=dev) // cnt
    j = torch.arange(nf, dtype=torch.int64, device=dev) % cnt
    fseg = seg.to(torch.int32)
    F = mss + 40
    out_off = torch.arange(nf + 1, dtype=torch.int64, device=dev) * F
    # (a)'s arrays: the expansion a caller without the offload makes, resident before the clock starts
    exp = {k: v[seg].contiguous() for k, v in sup.items()}
    exp["seq_num"] = wrap(sup["seq_num"][seg].to(torch.int64) + j * mss, 32, torch)
    keep = torch.where(j == cnt - 1, 0xFF, 0xFF ^ 0x09) & torch.where(j == 0, 0xFF, 0xFF ^ 0x80)
    exp["control"] = (sup["control"][seg].to(torch.int64) & keep).to(torch.uint8)
    eip = {"src": ip["src"].view(nsup, 4)[seg].reshape(-1).contiguous(),
           "dst": ip["dst"].view(nsup, 4)[seg].reshape(-1).contiguous(),
           "ident": wrap(ip["ident"][seg].to(torch.int64) + j, 16, torch), "ttl": ip["ttl"][seg].contiguous()}
    edoff = torch.arange(nf + 1, dtype=torch.int64, device=dev) * mss
    out_a = torch.empty(nf * F, dtype=torch.uint8, device=dev)
    out_b = torch.empty(nf * F, dtype=torch.uint8, device=dev)
    raw_a = torch.empty(nf, dtype=torch.int16, device=dev)
    raw_b = torch.empty(nf, dtype=torch.int16, device=dev)
    del seg, j, keep

    def a_frames():
        nsx.tx_ipv4_tcp_build_dev(eip, exp, data, edoff, out_a, out_off, raw=raw_a)

    def b_tso():
        nsx.tso_ipv4_tcp_build_dev(ip, sup, data, sdoff, dmss, first, fseg, out_b, out_off, raw=raw_b)

    a_frames()
    b_tso()
    torch.cuda.synchronize()
    same = bool(torch.equal(out_a, out_b)) and bool(torch.equal(raw_a, raw_b))
    print(f"parity {tag}: b_tso frames and raw sums vs a_frames: {'same' if same else 'MISMATCH'}", flush=True)
    if not same:
        raise SystemExit("segmentation offload's frames differ from the transmit pass's over the expanded arrays")
    written = nf * (F + 2)
    moved = {"a_frames": nf * (mss + TCP_B + IP4_B + 16) + 16 + written,        # per frame: fields, two offsets
             "b_tso": nsup * (L + TCP_B + IP4_B + 4 + 16) + nf * (4 + 8) + 24 + written}  # per frame: seg, out_off
    variants = [("a_frames", a_frames), ("b_tso", b_tso)]
    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:  # settle
        for _, step in variants:
            step()
        torch.cuda.synchronize()
    res = {name: [] for name, _ in variants}
    for r in range(rounds):
        for name, step in (variants if r % 2 == 0 else variants[::-1]):
            for _ in range(3):
                step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                step()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / launches)
        print(f"round {r}: " + " ".join(f"{k} {v[-1]:.5f}" for k, v in res.items()), flush=True)
    report(f"{tag} supers={nsup} frames={nf} mss={mss}", res, moved, "moved")
    ma, mb = statistics.median(res["a_frames"]), statistics.median(res["b_tso"])
    sa = (max(res["a_frames"]) - min(res["a_frames"])) / ma
    print(f"TSOAB {tag}: b_tso time vs a_frames {mb / ma:.4f} (a_frames' own spread {sa * 100:.2f}%); metadata bytes "
          f"read {(moved['b_tso'] - written - nsup * L) / 1e6:.1f} MB vs {(moved['a_frames'] - written - nf * mss) / 1e6:.1f} MB",
          flush=True)


def host_shape(nsup, cnt, mss, rounds):
    import numpy as np
    import nsx
    rng = np.random.default_rng(0x751)
    L, nf = cnt * mss, nsup * cnt
    dts = dict(src_port=np.uint16, dst_port=np.uint16, seq_num=np.uint32, ack_num=np.uint32, offset=np.uint8,
               control=np.uint8, window=np.uint16, urgent_ptr=np.uint16)
    sup = {k: rng.integers(0, 1 << (8 * np.dtype(dt).itemsize), nsup, dtype=np.uint64).astype(dt) for k, dt in dts.items()}
    sup["offset"][:] = 5
    ip = {"src": rng.integers(0, 256, (nsup, 4), dtype=np.uint8), "dst": rng.integers(0, 256, (nsup, 4), dtype=np.uint8),
          "ident": rng.integers(0, 1 << 16, nsup, dtype=np.uint64).astype(np.uint16),
          "ttl": rng.integers(0, 256, nsup, dtype=np.uint8)}
    sdoff = np.arange(nsup + 1, dtype=np.uint64) * np.uint64(L)
    smss = np.full(nsup, mss, np.uint32)
    first = nsx.tso_count_host(sdoff, smss)
    fseg, out_off = nsx.tso_layout_host(sdoff, smss, first, None, 20)
    assert int(first[-1]) == nf
    seg = fseg.astype(np.int64)
    j = np.arange(nf, dtype=np.int64) - first[:-1].astype(np.int64)[seg]
    exp = {k: np.ascontiguousarray(v[seg]) for k, v in sup.items()}
    exp["seq_num"] = (sup["seq_num"][seg].astype(np.int64) + j * mss).astype(np.uint32)
    keep = np.where(j == cnt - 1, 0xFF, 0xFF ^ 0x09) & np.where(j == 0, 0xFF, 0xFF ^ 0x80)
    exp["control"] = (sup["control"][seg] & keep).astype(np.uint8)
    eip = {"src": np.ascontiguousarray(ip["src"][seg]), "dst": np.ascontiguousarray(ip["dst"][seg]),
           "ident": (ip["ident"][seg].astype(np.int64) + j).astype(np.uint16), "ttl": np.ascontiguousarray(ip["ttl"][seg])}
    edoff = np.arange(nf + 1, dtype=np.uint64) * np.uint64(mss)
    total = int(out_off[-1])
    pd, po = nsx.PinnedBuffer(nsup * L), nsx.PinnedBuffer(total)
    pd.array[:] = rng.integers(0, 256, nsup * L, dtype=np.uint8)
    mem = {"pinned": (pd.array, po.array), "pageable": (pd.array.copy(), np.zeros(total, np.uint8))}

    def a_frames(m):
        d, o = mem[m]
        return nsx.tx_ipv4_tcp_build_host(eip, exp, d, edoff, out_off=out_off, out=o, num_gpus=1)

    def b_tso(m):
        d, o = mem[m]
        return nsx.tso_ipv4_tcp_build_host(ip, sup, d, sdoff, smss, frame_first=first, frame_seg=fseg, out_off=out_off,
                                           out=o, num_gpus=1)

    for m in mem:
        oa, ra = a_frames(m)
        oa, ra = oa.copy(), ra.copy()
        ob, rb = b_tso(m)
        same = np.array_equal(oa, ob) and np.array_equal(ra, rb)
        print(f"parity host {m}: b_tso frames and raw sums vs a_frames: {'same' if same else 'MISMATCH'}", flush=True)
        if not same:
            raise SystemExit("segmentation offload's host frames differ from the transmit pass's")
    h2d_a = nf * (mss + TCP_B + IP4_B + 16) + 16
    h2d_b = nsup * (L + TCP_B + IP4_B + 4 + 16) + nf * (4 + 8) + 24
    variants = [(f"{v}_{m}", fn, m) for m in mem for v, fn in (("a_frames", a_frames), ("b_tso", b_tso))]
    moved = {name: (h2d_a if name.startswith("a_") else h2d_b) for name, _, _ in variants}
    res = {name: [] for name, _, _ in variants}
    for r in range(rounds):
        for name, fn, m in (variants if r % 2 == 0 else variants[::-1]):
            fn(m)
            t0 = time.perf_counter()
            fn(m)
            res[name].append((time.perf_counter() - t0) * 1e3)
        print(f"round {r}: " + " ".join(f"{k} {v[-1]:.3f}" for k, v in res.items()), flush=True)
    report(f"host supers={nsup} frames={nf} mss={mss} images={total / 1e6:.1f}MB", res, moved, "H2D")
    for m in mem:
        ma, mb = statistics.median(res[f"a_frames_{m}"]), statistics.median(res[f"b_tso_{m}"])
        print(f"TSOAB host {m}: b_tso time vs a_frames {mb / ma:.4f}; H2D bytes {h2d_b / h2d_a:.4f} of a_frames' "
              f"(metadata {(h2d_b - nsup * L) / 1e6:.2f} MB vs {(h2d_a - nf * mss) / 1e6:.2f} MB); end-to-end "
              f"{(total + h2d_b) / mb / 1e6:.1f} vs {(total + h2d_a) / ma / 1e6:.1f} GB/s of PCIe traffic", flush=True)
    pd.free()
    po.free()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--shape", default="all", choices=["all", "dev", "jumbo", "host"])
    ap.add_argument("--host-n", type=int, default=2048)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.shape in ("all", "dev"):
        device_shape("dev45x1460", 23302, 45, 1460, a.rounds, a.launches)
        torch.cuda.empty_cache()
    if a.shape in ("all", "jumbo"):
        device_shape("jumbo7x8960", 37450, 7, 8960, a.rounds, a.launches)
        torch.cuda.empty_cache()
    if a.shape in ("all", "host"):
        host_shape(a.host_n, 45, 1460, a.rounds)


if __name__ == "__main__":
    main()
