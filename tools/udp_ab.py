#!/usr/bin/env python3
"""Same-process A/B of the UDP passes against their TCP twins, on one MI355X.

    python tools/udp_ab.py [--rounds 12] [--launches 10] [--n 1048576] [--out profiles/udp_ab.txt]

Transmit: n frames of 1500 B (IPv4) / 1520 B (IPv6) — a 1472 B UDP payload — and n frames of 80 B, built by
nsx_udp_tx_* beside nsx_tx_*_tcp_build_dev over frames of the same total length (option-less TCP: 12 payload bytes
fewer); and nsx_udp_uso_* cutting super-datagrams of 64 x 1472 B beside the per-frame call. Receive: nsx_udp_rx_* over
the UDP frames just built beside nsx_rx_*_tcp_verify_dev over the TCP frames of the same sizes.

The yardstick is the TCP leg of the same process. Every leg's output is checked before anything is timed: a sample of
frames byte for byte against the CPU restatement tests/_udp.py, segmentation against the per-frame call over the whole
buffer, and every frame through the receive passes (all valid). Then the legs run in interleaved rounds whose order
alternates, each round and leg `--launches` back-to-back calls between two HIP events. Per leg: median ms per call,
spread, bytes moved (read + written, the project's convention), GB/s, and the ratio to its TCP twin.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network-stack_amd"), os.path.join(ROOT, "tests")]

IPH = {4: 20, 6: 40}
SUPER = 64  # datagrams per super-datagram of the segmentation leg


def main():
    import nsx
    import torch
    import _udp
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "udp_ab.txt"))
    a = ap.parse_args()
    n = a.n - a.n % SUPER
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def rnd(count, bits, dtype, seed):
        t = torch.empty(count * 8, dtype=torch.uint8, device=dev)
        nsx.fill_splitmix64_dev(t, seed)
        return (t.view(torch.int64) & ((1 << bits) - 1)).to(dtype)

    data = torch.empty(n * 1472 + 64, dtype=torch.uint8, device=dev)
    nsx.fill_splitmix64_dev(data, 0x0DAB)
    idx = torch.arange(n + 1, dtype=torch.int64, device=dev)
    ports = {"src_port": rnd(n, 16, torch.int16, 1), "dst_port": rnd(n, 16, torch.int16, 2)}
    tcp = dict(ports, seq_num=rnd(n, 32, torch.int32, 3), ack_num=rnd(n, 32, torch.int32, 4),
               offset=torch.full((n,), 5, dtype=torch.uint8, device=dev), control=rnd(n, 8, torch.uint8, 5),
               window=rnd(n, 16, torch.int16, 6), urgent_ptr=rnd(n, 16, torch.int16, 7))
    ip = {4: {"src": rnd(n, 32, torch.int32, 8).view(torch.uint8), "dst": rnd(n, 32, torch.int32, 9).view(torch.uint8),
              "ident": rnd(n, 16, torch.int16, 10), "ttl": rnd(n, 8, torch.uint8, 11)},
          6: {"src": rnd(2 * n, 63, torch.int64, 12).view(torch.uint8),
              "dst": rnd(2 * n, 63, torch.int64, 13).view(torch.uint8), "ttl": rnd(n, 8, torch.uint8, 11),
              "tclass": rnd(n, 8, torch.uint8, 14), "flow": rnd(n, 20, torch.int32, 15)}}
    ipb = {4: 8 + 2 + 1, 6: 32 + 1 + 1 + 4}  # IP field bytes read per frame
    legs, moved, twin, bufs = [], {}, {}, {}
    for v in (4, 6):
        tx_u = nsx.udp_tx_ipv4_build_dev if v == 4 else nsx.udp_tx_ipv6_build_dev
        tx_t = nsx.tx_ipv4_tcp_build_dev if v == 4 else nsx.tx_ipv6_tcp_build_dev
        rx_u = nsx.udp_rx_ipv4_verify_dev if v == 4 else nsx.udp_rx_ipv6_verify_dev
        rx_t = nsx.rx_ipv4_tcp_verify_dev if v == 4 else nsx.rx_ipv6_tcp_verify_dev
        uso = nsx.udp_uso_ipv4_build_dev if v == 4 else nsx.udp_uso_ipv6_build_dev
        for size, F in (("big", 1472 + 28 + (20 if v == 6 else 0)), ("small", 80)):
            pu, pt = F - IPH[v] - 8, F - IPH[v] - 20  # payload bytes: UDP, TCP
            off = idx * F
            du, dt = idx * pu, idx * pt
            # each leg is given the extent of its own payloads: both passes size their wave tasks from data_bytes / n
            dau, dat = data[:n * pu + 64], data[:n * pt + 64]
            ou = torch.zeros(n * F, dtype=torch.uint8, device=dev)
            ot = torch.zeros(n * F, dtype=torch.uint8, device=dev)
            ru, rt = torch.zeros(n, dtype=torch.int16, device=dev), torch.zeros(n, dtype=torch.int16, device=dev)
            mask = torch.zeros((n + 63) // 64, dtype=torch.int64, device=dev)
            r2 = torch.zeros(n, dtype=torch.int16, device=dev)
            k = f"ipv{v}_{size}"
            bufs[k] = (ou, ot, off, du, pu, ru)
            legs += [(f"udp_tx_{k}", lambda tx_u=tx_u, v=v, dau=dau, du=du, ou=ou, off=off, ru=ru:
                      tx_u(ip[v], ports, dau, du, ou, off, raw=ru)),
                     (f"tcp_tx_{k}", lambda tx_t=tx_t, v=v, dat=dat, dt=dt, ot=ot, off=off, rt=rt:
                      tx_t(ip[v], tcp, dat, dt, ot, off, raw=rt)),
                     (f"udp_rx_{k}", lambda rx_u=rx_u, ou=ou, off=off, mask=mask, r2=r2:
                      rx_u(ou, off, mask=mask, udp_raw=r2)),
                     (f"tcp_rx_{k}", lambda rx_t=rx_t, ot=ot, off=off, mask=mask, r2=r2:
                      rx_t(ot, off, mask=mask, tcp_raw=r2))]
            moved[f"udp_tx_{k}"] = n * (pu + 4 + 16 + ipb[v] + F + 2)
            moved[f"tcp_tx_{k}"] = n * (pt + 18 + 16 + ipb[v] + F + 2)
            moved[f"udp_rx_{k}"] = moved[f"tcp_rx_{k}"] = n * (F + 8 + 2) + n // 8
            twin[f"udp_tx_{k}"], twin[f"udp_rx_{k}"] = f"tcp_tx_{k}", f"tcp_rx_{k}"
        # segmentation: n / SUPER super-datagrams of SUPER x 1472 B, the frames of the big leg
        ns = n // SUPER
        F = 1472 + 8 + IPH[v]
        sup_ip = {kk: t.view(n, -1)[::SUPER].contiguous().view(-1) for kk, t in ip[v].items()}
        if v == 4:  # idents that count up inside a super-datagram are what the per-frame leg below is given too
            sup_ip["ident"] = torch.zeros(ns, dtype=torch.int16, device=dev)
        sup_ports = {kk: t[::SUPER].contiguous() for kk, t in ports.items()}
        s_off = torch.arange(ns + 1, dtype=torch.int64, device=dev) * (SUPER * 1472)
        gso = torch.full((ns,), 1472, dtype=torch.int32, device=dev)
        first = torch.arange(ns + 1, dtype=torch.int64, device=dev) * SUPER
        seg = (torch.arange(n, dtype=torch.int64, device=dev) // SUPER).to(torch.int32)
        os_ = torch.zeros(n * F, dtype=torch.uint8, device=dev)
        rs = torch.zeros(n, dtype=torch.int16, device=dev)
        off = idx * F
        k = f"ipv{v}_big"
        bufs[f"uso_{v}"] = (os_, rs, sup_ip, sup_ports)
        legs.append((f"udp_uso_{k}", lambda uso=uso, sup_ip=sup_ip, sup_ports=sup_ports, s_off=s_off, gso=gso,
                     first=first, seg=seg, os_=os_, off=off, rs=rs:
                     uso(sup_ip, sup_ports, data, s_off, gso, first, seg, os_, off, raw=rs)))
        moved[f"udp_uso_{k}"] = n * (1472 + 4 + 8 + F + 2) + ns * (4 + 16 + 4 + 8 + ipb[v])
        twin[f"udp_uso_{k}"] = f"udp_tx_{k}"

    # ---- every leg's output before anything is timed ----
    for _, step in legs:  # the tx legs come before the rx legs of their buffers
        step()
    torch.cuda.synchronize()
    for v in (4, 6):
        for size in ("big", "small"):
            k = f"ipv{v}_{size}"
            ou, ot, off, du, pu, ru = bufs[k]
            F = int(off[1])
            for lo in (0, n // 2 - 100, n - 200):  # 200 frames at the start, the middle and the end against the model
                c = _udp.Case.__new__(_udp.Case)
                c.ipver, c.n = v, 200
                d0 = int(du[lo])
                c.data = data[d0:int(du[lo + 200])].cpu().numpy()
                c.data_off = (du[lo:lo + 201].cpu().numpy() - d0).astype(np.uint64)
                c.lo, c.hi = c.data_off[:-1], c.data_off[1:]
                c.ports = {kk: t[lo:lo + 200].cpu().numpy().view(np.uint16) for kk, t in ports.items()}
                al = 4 if v == 4 else 16
                c.ip = {kk: t.view(n, -1)[lo:lo + 200].cpu().numpy() for kk, t in ip[v].items()}
                c.ip = {"src": c.ip["src"].reshape(200, al), "dst": c.ip["dst"].reshape(200, al),
                        "ident": c.ip.get("ident", np.zeros((200, 1), np.int16)).reshape(-1).view(np.uint16),
                        "ttl": c.ip["ttl"].reshape(-1), "tclass": c.ip.get("tclass", np.zeros(200, np.uint8)).reshape(-1),
                        "flow": c.ip.get("flow", np.zeros((200, 1), np.int32)).reshape(-1).view(np.uint32)}
                want, wraw = _udp.expected(c, c.packed())
                got = ou[lo * F:(lo + 200) * F].cpu().numpy()
                if not (np.array_equal(got, want) and np.array_equal(ru[lo:lo + 200].cpu().numpy().view(np.uint16), wraw)):
                    raise SystemExit(f"udp_tx_{k}: frames {lo}..{lo + 200} differ from the model")
            full = -1 if n % 64 == 0 else None
            for name, fn, buf in (("udp_rx", nsx.udp_rx_ipv4_verify_dev if v == 4 else nsx.udp_rx_ipv6_verify_dev, ou),
                                  ("tcp_rx", nsx.rx_ipv4_tcp_verify_dev if v == 4 else nsx.rx_ipv6_tcp_verify_dev, ot)):
                m = fn(buf, off)
                torch.cuda.synchronize()
                if full is not None and not bool((m == full).all()):
                    raise SystemExit(f"{name}_{k}: not every frame verifies")
            other = nsx.udp_rx_ipv4_verify_dev if v == 4 else nsx.udp_rx_ipv6_verify_dev
            if bool(other(ot, off).any()):
                raise SystemExit(f"udp_rx over the TCP frames of {k}: mask not zero")
            say(f"checked {k}: udp_tx against the model (600 frames), udp_rx / tcp_rx all valid, udp_rx over TCP frames 0")
        # segmentation == the per-frame call given the same fields per frame
        os_, rs, sup_ip, sup_ports = bufs[f"uso_{v}"]
        F = 1472 + 8 + IPH[v]
        ipf = {kk: t.view(n // SUPER, -1).repeat_interleave(SUPER, 0).contiguous().view(-1) for kk, t in sup_ip.items()}
        if v == 4:
            ipf["ident"] = (torch.arange(n, device=dev) % SUPER).to(torch.int16)
        pf = {kk: t.repeat_interleave(SUPER).contiguous() for kk, t in sup_ports.items()}
        o2, r2 = torch.zeros_like(os_), torch.zeros_like(rs)
        (nsx.udp_tx_ipv4_build_dev if v == 4 else nsx.udp_tx_ipv6_build_dev)(ipf, pf, data, idx * 1472, o2, idx * F, raw=r2)
        torch.cuda.synchronize()
        if not (bool(torch.equal(os_, o2)) and bool(torch.equal(rs, r2))):
            raise SystemExit(f"udp_uso_ipv{v}: differs from the per-frame call")
        say(f"checked udp_uso_ipv{v}_big: byte for byte the per-frame call over the expanded batch")
        del o2, r2, ipf, pf

    t_end = time.perf_counter() + 1.0
    while time.perf_counter() < t_end:  # settle
        for _, step in legs:
            step()
        torch.cuda.synchronize()
    res = {name: [] for name, _ in legs}
    for r in range(a.rounds):
        for name, step in (legs if r % 2 == 0 else legs[::-1]):
            for _ in range(2):
                step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                step()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / a.launches)
    med = {k: statistics.median(v) for k, v in res.items()}
    for name, _ in legs:
        v = sorted(res[name])
        say(f"UDPAB n={n} {name:20s} median {med[name]:.5f} ms/call  min {v[0]:.5f} max {v[-1]:.5f} spread "
            f"{(v[-1] - v[0]) / med[name] * 100:.2f}%  moved {moved[name] / 1e6:.1f} MB  "
            f"{moved[name] / (med[name] * 1e-3) / 1e9:.1f} GB/s")
    for name, t in twin.items():
        say(f"UDPAB {name:20s} vs {t:20s}: time {med[name] / med[t]:.4f}  rate "
            f"{(moved[name] / med[name]) / (moved[t] / med[t]):.4f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# tools/udp_ab.py on one MI355X, one process: {a.rounds} rounds x {a.launches} calls per leg, order "
                f"alternating\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
