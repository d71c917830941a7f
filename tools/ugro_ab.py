#!/usr/bin/env python3
"""Same-process A/B of UDP receive coalescing against its TCP twins and a plain copy, on one MI355X.

    python tools/ugro_ab.py [--rounds 10] [--launches 5] [--n 1048576] [--out profiles/ugro_ab.txt]

Two sizes, each for IPv4 and IPv6: n UDP frames of 1500 B (IPv6: 1520 B — a 1472 B payload) and n UDP frames of 80 B
(52 / 32 B of payload), made on the device by nsx_udp_uso_* as runs of 64 datagrams of one flow. Per size and version
five legs run in interleaved rounds whose order alternates, `--launches` back-to-back calls between two HIP events:
  ugro       nsx_ugro_ipvX_dev over the UDP frames (its five launches);
  ugro_flow  nsx_ugro_flow_ipvX_dev over the same frames (key pass and radix sort first);
  gro        nsx_gro_ipvX_tcp_dev over n option-less TCP frames of the same payload bytes, made by nsx_tso_* as runs
             of 64 segments (frames 12 B longer: the yardstick);
  gro_flow   nsx_gro_flow_ipvX_tcp_dev over those;
  copy       one device-to-device copy of the payload volume (n x payload bytes).
Before anything is timed the outputs are checked: n_super, frame_cnt, gso / mss and — for the adjacent forms — every
payload byte equal the batch the frames were cut from. Bytes moved = frame bytes read + payload bytes written (the
copy: twice the payload), the project's convention.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network-stack_amd")]

RUN = 64  # frames per run
IPH = {4: 20, 6: 40}


def config(tag, v, pay, n, rounds, launches, say):
    import nsx
    import torch
    dev = torch.device("cuda", 0)
    ns, alen = n // RUN, 4 if v == 4 else 16

    def rnd(count, bits, dtype, seed):
        t = torch.empty(count * 8, dtype=torch.uint8, device=dev)
        nsx.fill_splitmix64_dev(t, seed)
        return (t.view(torch.int64) & ((1 << bits) - 1)).to(dtype)

    data = torch.empty(n * pay, dtype=torch.uint8, device=dev)
    nsx.fill_splitmix64_dev(data, 0x06AB + pay)
    ip = {"src": rnd(ns * alen // 4, 32, torch.int32, 1).view(torch.uint8),
          "dst": rnd(ns * alen // 4, 32, torch.int32, 2).view(torch.uint8),
          "ident": torch.zeros(ns, dtype=torch.int16, device=dev), "ttl": rnd(ns, 8, torch.uint8, 3),
          "tclass": torch.zeros(ns, dtype=torch.uint8, device=dev), "flow": rnd(ns, 20, torch.int32, 4)}
    ports = {"src_port": rnd(ns, 16, torch.int16, 5), "dst_port": rnd(ns, 16, torch.int16, 6)}
    tcp = dict(ports, seq_num=rnd(ns, 32, torch.int32, 7), ack_num=rnd(ns, 32, torch.int32, 8),
               offset=torch.full((ns,), 0x50, dtype=torch.uint8, device=dev),  # data offset 5, as on the wire
               control=torch.full((ns,), 0x10, dtype=torch.uint8, device=dev), window=rnd(ns, 16, torch.int16, 9),
               urgent_ptr=torch.zeros(ns, dtype=torch.int16, device=dev))
    s_off = torch.arange(ns + 1, dtype=torch.int64, device=dev) * (RUN * pay)
    per = torch.full((ns,), pay, dtype=torch.int32, device=dev)
    first = torch.arange(ns + 1, dtype=torch.int64, device=dev) * RUN
    seg = (torch.arange(n, dtype=torch.int64, device=dev) // RUN).to(torch.int32)
    idx = torch.arange(n + 1, dtype=torch.int64, device=dev)
    fu, ft = pay + IPH[v] + 8, pay + IPH[v] + 20
    assert fu % 4 == 0 and ft % 4 == 0  # the builds' slots are the receive passes' offsets
    off_u, off_t = idx * fu, idx * ft
    udp_frames = torch.empty(n * fu, dtype=torch.uint8, device=dev)
    tcp_frames = torch.empty(n * ft, dtype=torch.uint8, device=dev)
    (nsx.udp_uso_ipv4_build_dev if v == 4 else nsx.udp_uso_ipv6_build_dev)(
        ip, ports, data, s_off, per, first, seg, udp_frames, off_u)
    (nsx.tso_ipv4_tcp_build_dev if v == 4 else nsx.tso_ipv6_tcp_build_dev)(
        ip, tcp, data, s_off, per, first, seg, tcp_frames, off_t)
    mask_u = (nsx.udp_rx_ipv4_verify_dev if v == 4 else nsx.udp_rx_ipv6_verify_dev)(udp_frames, off_u)
    mask_t = (nsx.rx_ipv4_tcp_verify_dev if v == 4 else nsx.rx_ipv6_tcp_verify_dev)(tcp_frames, off_t)
    torch.cuda.synchronize()
    if not (bool((mask_u == -1).all()) and bool((mask_t == -1).all())):
        raise SystemExit(f"{tag}: not every frame verifies")
    fns = {"ugro": (getattr(nsx, f"ugro_ipv{v}_dev"), udp_frames, off_u, mask_u, nsx.ugro_work_bytes(n)),
           "ugro_flow": (getattr(nsx, f"ugro_flow_ipv{v}_dev"), udp_frames, off_u, mask_u, nsx.ugro_flow_work_bytes(n)),
           "gro": (getattr(nsx, f"gro_ipv{v}_tcp_dev"), tcp_frames, off_t, mask_t, nsx.gro_work_bytes(n)),
           "gro_flow": (getattr(nsx, f"gro_flow_ipv{v}_tcp_dev"), tcp_frames, off_t, mask_t,
                        nsx.gro_flow_work_bytes(n))}
    legs, moved = [], {}
    for name, (fn, frames, off, mask, need) in fns.items():
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        out = fn(frames, off, mask, work=work)
        torch.cuda.synchronize()
        k = int(out["n_super"].item())
        ok = k == ns and bool((out["frame_cnt"][:k] == RUN).all()) and int(out["data_off"][k].item()) == n * pay and \
            bool((out["gso" if name.startswith("u") else "mss"][:k] == pay).all())
        if ok and not name.endswith("flow"):
            ok = bool(torch.equal(out["data"][:n * pay], data)) and bool(torch.equal(out["data_off"][:k + 1], s_off))
        if not ok:
            raise SystemExit(f"{tag} {name}: the output is not the batch the frames were cut from")
        kw = {"order": out.pop("order")} if name.endswith("flow") else {}
        legs.append((name, lambda fn=fn, frames=frames, off=off, mask=mask, out=out, work=work, kw=kw:
                     fn(frames, off, mask, out=out, work=work, **kw)))
        moved[name] = frames.numel() + n * pay
    dst = torch.empty_like(data)
    legs.append(("copy", lambda: dst.copy_(data)))
    moved["copy"] = 2 * n * pay
    say(f"checked {tag}: {n} frames, {ns} runs of {RUN} x {pay} B; all four calls give the batch back")
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
    med = {k: statistics.median(x) for k, x in res.items()}
    for name, _ in legs:
        x = sorted(res[name])
        say(f"UGROAB {tag} {name:10s} median {med[name]:.5f} ms/call  min {x[0]:.5f} max {x[-1]:.5f} spread "
            f"{(x[-1] - x[0]) / med[name] * 100:.2f}%  moved {moved[name] / 1e6:.1f} MB  "
            f"{moved[name] / (med[name] * 1e-3) / 1e9:.1f} GB/s")
    for a, b in (("ugro", "gro"), ("ugro_flow", "gro_flow"), ("ugro", "copy"), ("gro", "copy")):
        say(f"UGROAB {tag} {a:10s} vs {b:9s}: time {med[a] / med[b]:.4f}  rate "
            f"{(moved[a] / med[a]) / (moved[b] / med[b]):.4f}")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ugro_ab.txt"))
    a = ap.parse_args()
    n = a.n - a.n % RUN
    torch.cuda.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for size, frame in (("big", 1500), ("small", 80)):
        for v in (4, 6):
            pay = frame - 28 if size == "big" else frame - IPH[v] - 8
            config(f"ipv{v}_{size}", v, pay, n, a.rounds, a.launches, say)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# tools/ugro_ab.py on one MI355X, one process: {a.rounds} rounds x {a.launches} calls per leg, order "
                f"alternating\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
