#!/usr/bin/env python3
"""Same-process timing of the in-place NAT rewrite (nsx_nat_*_tcp_rewrite_dev) against the fused receive pass
(nsx_rx_*_tcp_verify_dev) over the same frames: what changing ~16 header bytes per frame costs next to touching
every byte of it, which is what a rewrite through parse / GRO and the transmit pass would have to do at least once.

    python tools/nat_ab.py [--rounds 10] [--launches 10] [--ipver 0|4|6] [--rules 65536] [--hit 0.9]
                           [--out profiles/nat_ab.txt]

Batch: bench.py's workload 10 (IPv4: 1M frames of 40-1500 B, densely packed at odd starts, 1 in 1000 corrupted) and
its IPv6 twin, workload 11, built on the device as the benchmark builds them. Every frame then gets the address /
port tuple of one of rules / hit flows (drawn uniformly; the checksums are filled again by the library's own ragged
kernel, and the same 1 in 1000 frames corrupted again), and the table holds rules for the first `rules` flows: about
`hit` of the frames hit, less the frames that do not verify and those whose TTL is 0.
The rewrite is in place, so a second call over the same buffer would find other tuples than the first. The rules are
therefore made in pairs, flow 2k -> flow 2k+1 and back, and ttl_dec is 0: every call translates the same frames,
between two tuples that are both in the table, and two calls give the original buffer back — which is checked, byte
for byte, before timing, together with the receive pass's mask after one call (the same as before it: the incremental
update keeps valid frames valid and broken ones broken) and the hit count.
Three legs in interleaved rounds whose order alternates, `--launches` back-to-back calls bracketed by HIP events on
the launch stream (an even number, so that the buffer is the original again after each bracket):
  nat   nsx_nat_*_tcp_rewrite_dev with the receive pass's mask;
  rx    nsx_rx_*_tcp_verify_dev over the same buffer (the yardstick: one read of every frame byte);
  nat2  the nat leg again — the difference between the two is the run-to-run spread of this process.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network-stack_amd"), os.path.join(ROOT, "tools")]

LEGS = ("nat", "rx", "nat2")


def set_tuples(frames, tuples, ipver, torch, nsx):
    """Frame i's addresses and ports := tuples[i]; both checksum fields filled again as bench.build_rx_frames fills
    them (the frames have IHL 5 / no extension headers), and the benchmark's 1 in 1000 frames corrupted again."""
    buf, d_offs = frames["buf"], frames["d_offs"]
    dev = buf.device
    st = d_offs[:-1]
    ln = d_offs[1:] - st
    iph, a0, alen = (20, 12, 4) if ipver == 4 else (40, 8, 16)
    na = 2 * alen
    buf[(st[:, None] + a0 + torch.arange(na, device=dev)).reshape(-1)] = tuples[:, :na].reshape(-1)
    buf[(st[:, None] + iph + torch.arange(4, device=dev)).reshape(-1)] = tuples[:, na:].reshape(-1)
    fields = ((10, 11) if ipver == 4 else ()) + (iph + 16, iph + 17)
    for k in fields:
        buf[st + k] = 0
    src, dst = tuples[:, :alen].reshape(-1).contiguous(), tuples[:, alen:na].reshape(-1).contiguous()
    tcp_len = (ln - iph).to(torch.int32)
    pseudo = (nsx.pseudo_ipv4_partial_dev if ipver == 4 else nsx.pseudo_ipv6_partial_dev)(src, dst, tcp_len, 6)
    spans = torch.cat([torch.stack([st, st + iph], 1).reshape(-1), d_offs[-1:]])
    part2 = torch.stack([torch.zeros_like(pseudo), pseudo], 1).reshape(-1)
    fld = ~(nsx.ragged_dev(buf, spans, partial=part2).to(torch.int32)) & 0xFFFF
    if ipver == 4:
        buf[st + 10], buf[st + 11] = (fld[0::2] >> 8).to(torch.uint8), (fld[0::2] & 0xFF).to(torch.uint8)
    buf[st + iph + 16], buf[st + iph + 17] = (fld[1::2] >> 8).to(torch.uint8), (fld[1::2] & 0xFF).to(torch.uint8)
    buf[st[::1000] + iph + 10] ^= 1
    torch.cuda.synchronize()


def run(ipver, rounds, launches, rules, hit, emit):
    import numpy as np
    import bench
    import nsx
    import torch
    dev = torch.device("cuda", 0)
    cfg = bench.WORKLOADS[10 if ipver == 4 else 11]
    frames = bench.build_rx_frames(cfg, cfg["seed"], dev)
    n, fbytes = cfg["n"], frames["bytes"]
    buf, d_offs = frames["buf"], frames["d_offs"]
    rng = np.random.default_rng(0x4A7 + ipver)
    tb = nsx.NAT_TUPLE_BYTES[ipver]
    flows = max(int(round(rules / hit)), rules)
    pool = rng.integers(0, 256, (flows, tb), dtype=np.uint8)
    assert np.unique(pool, axis=0).shape[0] == flows
    set_tuples(frames, torch.from_numpy(pool).to(dev)[torch.from_numpy(rng.integers(0, flows, n)).to(dev)], ipver,
               torch, nsx)
    match = pool[:rules]
    new = match.reshape(rules // 2, 2, tb)[:, ::-1].reshape(rules, tb)  # flow 2k <-> flow 2k + 1
    slots = nsx.nat_table_slots(rules)
    table = torch.from_numpy(nsx.nat_table_build_host(ipver, match, new, slots)).to(dev)
    rx_fn = nsx.rx_ipv4_tcp_verify_dev if ipver == 4 else nsx.rx_ipv6_tcp_verify_dev
    nat_fn = nsx.nat_ipv4_tcp_rewrite_dev if ipver == 4 else nsx.nat_ipv6_tcp_rewrite_dev
    mask = rx_fn(buf, d_offs).clone()
    mask2 = torch.empty_like(mask)
    hits = torch.empty_like(mask)
    tag = f"v{ipver}"

    # parity: one call keeps the receive pass's mask, translates about `hit` of the frames and changes the buffer;
    # a second call gives the original bytes back
    orig = buf.clone()
    nat_fn(buf, d_offs, mask, table, slots, ttl_dec=0, hit=hits)
    rx_fn(buf, d_offs, mask=mask2)
    torch.cuda.synchronize()
    bits = lambda m: int(sum(bin(int(w) & (2**64 - 1)).count("1") for w in m.cpu().numpy()))  # noqa: E731
    nhit, nvalid = bits(hits), bits(mask)
    changed = int((buf != orig).sum().item())
    ok = bool(torch.equal(mask, mask2)) and changed > 0
    nat_fn(buf, d_offs, mask, table, slots, ttl_dec=0, hit=hits)
    torch.cuda.synchronize()
    ok = ok and bool(torch.equal(buf, orig)) and bits(hits) == nhit
    del orig
    emit(f"parity {tag}: {n} frames ({fbytes / 1e6:.1f} MB), {nvalid} verify, {rules} rules in {slots} slots "
         f"({table.numel() / 1e6:.1f} MB), {nhit} translated ({nhit / n:.4f}), {changed} bytes changed by one call, "
         f"receive mask after it and the buffer after two: {'same' if ok else 'MISMATCH'}")
    if not ok:
        raise SystemExit("the rewrite did not keep the receive pass's mask or did not give the buffer back")
    torch.cuda.empty_cache()

    steps = {"nat": lambda: nat_fn(buf, d_offs, mask, table, slots, ttl_dec=0, hit=hits),
             "rx": lambda: rx_fn(buf, d_offs, mask=mask2)}
    steps["nat2"] = steps["nat"]
    legs = [(name, steps[name]) for name in LEGS]
    t_end = time.perf_counter() + 0.5
    while time.perf_counter() < t_end:  # settle
        for _, step in legs:
            step()
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
        rate = fbytes / (med[name] * 1e-3) / 1e9
        emit(f"NATAB {tag} {name:4s} median {med[name]:.5f} ms/call  min {v[0]:.5f} max {v[-1]:.5f}  frame bytes "
             f"{fbytes / 1e6:.1f} MB  {rate:.1f} GB/s of frame bytes  frac of HBM peak "
             f"{rate / bench.HBM_PEAK_GBPS:.4f}")
    base = min(med["nat"], med["nat2"])
    spread = abs(med["nat"] - med["nat2"]) / base
    emit(f"NATAB {tag}: rewrite {base:.5f} ms, receive pass {med['rx']:.5f} ms: rewrite / receive pass "
         f"{base / med['rx']:.4f}; {base * 1e6 / n:.3f} ns per frame, {base * 1e6 / max(nhit, 1):.3f} ns per "
         f"translated frame; spread between the two nat legs {spread * 100:.2f}%")
    torch.cuda.synchronize()
    mask2.zero_()
    rx_fn(buf, d_offs, mask=mask2)
    torch.cuda.synchronize()
    if not torch.equal(mask, mask2):
        raise SystemExit("the receive pass's mask changed during the timed calls")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--ipver", type=int, default=0, choices=[0, 4, 6])
    ap.add_argument("--rules", type=int, default=1 << 16)
    ap.add_argument("--hit", type=float, default=0.9, help="share of the frames whose tuple has a rule")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nat_ab.txt"))
    a = ap.parse_args()
    if a.launches % 2 or a.rules % 2 or a.rules < 2 or not 0.0 < a.hit <= 1.0:
        ap.error("--launches and --rules must be even (the rules come in pairs), 0 < --hit <= 1")
    torch.cuda.set_device(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("In-place NAT rewrite (nsx_nat_ipv4_tcp_rewrite_dev / nsx_nat_ipv6_tcp_rewrite_dev) against the fused receive "
         "pass over the same frames, one MI355X.")
    emit(f"  python tools/nat_ab.py --rounds {a.rounds} --launches {a.launches} --rules {a.rules} --hit {a.hit}")
    emit("Same process, three legs in interleaved rounds whose order alternates, back-to-back calls bracketed by HIP "
         "events: nat = the rewrite with the receive pass's mask (rules in pairs A <-> B, ttl_dec 0, so every call "
         "translates the same frames), rx = nsx_rx_*_tcp_verify_dev over the same buffer, nat2 = nat again.")
    emit("")
    for ipver in (4, 6):
        if a.ipver in (0, ipver):
            run(ipver, a.rounds, a.launches, a.rules, a.hit, emit)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
