#!/usr/bin/env python3
"""Same-process A/B of the fused transmit pass against the two-launch sender sequence it replaces, on bench
workload 6's shape (1M option-less segments, 1480 B payloads at 4-aligned offsets).

    python tools/tx_ab.py [--rounds 20] [--launches 20] [--n 1048576]

(a) the existing sender sequence: nsx_pseudo_ipv4_partial_dev + nsx_tcp_build_dev (TCP images only; timed as
    pseudo, build, and the two back to back);
(b) nsx_tx_ipv4_tcp_build_dev over the same inputs (whole IPv4 datagrams, no partials array), and the IPv6 form.

Builds the workload once (bench.build_workload), checks that (b)'s TCP parts and raw sums are (a)'s, settles the
clocks, then times every variant in interleaved rounds whose order alternates (each round and variant: `--launches`
back-to-back calls bracketed by HIP events on the launch stream). Prints per variant the median time per call, its
spread over the rounds, the bytes the call moves and the rate. The margin for any comparison is the spread of (a)
itself in this process.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network-stack_amd")]


def main():
    import bench
    import nsx
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--n", type=int, default=0, help="override workload 6's segment count")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cfg = dict(bench.WORKLOADS[6])
    if a.n:
        cfg["n"] = a.n
    w = bench.build_workload(cfg, 0, dev)
    n, P = cfg["n"], cfg["payload"]
    W = P + 20
    f, data, data_off, addrs = w["fields"], w["data"], w["data_off"], w["addrs"]
    g = torch.Generator(device=dev).manual_seed(cfg["seed"] + 1)
    idx = torch.arange(n + 1, dtype=torch.int64, device=dev)
    ip4 = {"src": addrs[0].reshape(-1).contiguous(), "dst": addrs[1].reshape(-1).contiguous(),
           "ident": torch.randint(0, 1 << 16, (n,), generator=g, device=dev, dtype=torch.int64).to(torch.int16),
           "ttl": torch.randint(0, 256, (n,), generator=g, device=dev, dtype=torch.int64).to(torch.uint8)}
    a6 = torch.randint(0, 256, (2, n, 16), generator=g, device=dev, dtype=torch.int64).to(torch.uint8)
    ip6 = {"src": a6[0].reshape(-1).contiguous(), "dst": a6[1].reshape(-1).contiguous(), "ttl": ip4["ttl"],
           "tclass": torch.randint(0, 256, (n,), generator=g, device=dev, dtype=torch.int64).to(torch.uint8),
           "flow": torch.randint(0, 1 << 20, (n,), generator=g, device=dev, dtype=torch.int64).to(torch.int32)}
    off4, off6 = idx * (W + 20), idx * (W + 40)
    out4 = torch.empty(n * (W + 20), dtype=torch.uint8, device=dev)
    out6 = torch.empty(n * (W + 40), dtype=torch.uint8, device=dev)
    raw4 = torch.empty(n, dtype=torch.int16, device=dev)
    raw6 = torch.empty(n, dtype=torch.int16, device=dev)
    wire_len = torch.full((n,), W, dtype=torch.int32, device=dev)
    part = w["part"]

    def pseudo():
        nsx.pseudo_ipv4_partial_dev(ip4["src"], ip4["dst"], wire_len, 6, out=part)

    build = w["step_for"](None)

    def seq():
        pseudo()
        build()

    def tx4():
        nsx.tx_ipv4_tcp_build_dev(ip4, f, data, data_off, out4, off4, raw=raw4)

    def tx6():
        nsx.tx_ipv6_tcp_build_dev(ip6, f, data, data_off, out6, off6, raw=raw6)

    # bytes one call moves: per segment the payload, 18 B of TCP fields, two 8 B offsets (+ 16 B of array ends)
    common = P + 18 + 16
    moved = {
        "a_pseudo": n * (8 + 4 + 4),                       # addresses + length read, partial written
        "a_build": n * (common + 4 + W + 2) + 16,          # + partial read; image + raw sum written
        "b_tx_ipv4": n * (common + 8 + 3 + W + 20 + 2) + 16,   # + addresses, ident, ttl read; header written
        "b_tx_ipv6": n * (common + 32 + 6 + W + 40 + 2) + 16,  # + addresses, ttl, tclass, flow read; header written
    }
    moved["a_seq"] = moved["a_pseudo"] + moved["a_build"]
    variants = [("a_pseudo", pseudo), ("a_build", build), ("a_seq", seq), ("b_tx_ipv4", tx4), ("b_tx_ipv6", tx6)]

    # (b) computes what (a) computes: the TCP part of every datagram is (a)'s image with its own checksum field
    # (IPv4: the same pseudo-header, so identical bytes and raw sums)
    seq()
    tx4()
    tx6()
    torch.cuda.synchronize()
    same = bool(torch.equal(out4.view(n, W + 20)[:, 20:], w["wire"].view(n, W))) and bool(torch.equal(raw4, w["out"]))
    print(f"parity b_tx_ipv4 TCP parts and raw sums vs a_build: {'same' if same else 'MISMATCH'}", flush=True)
    if not same:
        raise SystemExit("the transmit pass's TCP images differ from nsx_tcp_build_dev's")
    d6 = out6.view(n, W + 40)[:, 40:] != w["wire"].view(n, W)
    d6[:, 16:18] = False  # another pseudo-header: only the checksum field may differ
    print(f"parity b_tx_ipv6 TCP parts vs a_build (checksum field aside): {'same' if not bool(d6.any()) else 'MISMATCH'}",
          flush=True)
    if bool(d6.any()):
        raise SystemExit("the IPv6 transmit pass's TCP images differ from nsx_tcp_build_dev's")

    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:  # settle
        for _, step in variants:
            step()
        torch.cuda.synchronize()
    res = {name: [] for name, _ in variants}
    for r in range(a.rounds):
        for name, step in (variants if r % 2 == 0 else variants[::-1]):
            for _ in range(3):
                step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                step()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / a.launches)
        print(f"round {r}: " + " ".join(f"{k} {v[-1]:.5f}" for k, v in res.items()), flush=True)
    for name, _ in variants:
        v = sorted(res[name])
        med = statistics.median(v)
        q1, q3 = v[len(v) // 4], v[(3 * len(v)) // 4]
        print(f"TXAB n={n} payload={P} {name:10s} median {med:.5f} ms/call  min {v[0]:.5f} max {v[-1]:.5f} "
              f"iqr {q3 - q1:.5f} spread {(v[-1] - v[0]) / med * 100:.2f}%  moved {moved[name] / 1e6:.1f} MB  "
              f"{moved[name] / (med * 1e-3) / 1e9:.1f} GB/s  frac of HBM peak "
              f"{moved[name] / (med * 1e-3) / 1e9 / bench.HBM_PEAK_GBPS:.4f}", flush=True)
    ab, a_seq = statistics.median(res["a_build"]), statistics.median(res["a_seq"])
    for name in ("b_tx_ipv4", "b_tx_ipv6"):
        med = statistics.median(res[name])
        print(f"TXAB {name}: time vs a_seq {med / a_seq:.4f}, vs a_build {med / ab:.4f}; rate vs a_build's "
              f"{(moved[name] / med) / (moved['a_build'] / ab):.4f}", flush=True)


if __name__ == "__main__":
    main()
