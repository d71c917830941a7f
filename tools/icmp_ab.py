#!/usr/bin/env python3
"""Same-process timing of the ICMP family against a yardstick per leg, on one MI355X.

    python tools/icmp_ab.py [--rounds 10] [--launches 5] [--scale 1] [--out profiles/icmp_ab.txt]

1 M frames (--scale divides the count: rehearsals) per IP version and size: 1500 B IPv4 / 1520 B IPv6, and 80 B. The
frames are UDP datagrams built on the device by nsx_udp_tx_*_build_dev with random unicast addresses, and ICMP echo
requests of the same lengths made from them (protocol 1 / 58, type 8 / 128, the checksums filled by the library's own
fixed-stride kernel). Per size and version six legs run in interleaved rounds whose order alternates:
  err     nsx_icmp_err_*_dev with every frame requested ("time exceeded") over the UDP frames;
  copy    hipMemcpyAsync, device to device, of the bytes err writes — its yardstick, as tools/frag_ab.py's;
  rx      nsx_icmp_rx_*_verify_dev over the echo requests;
  udp_rx  nsx_udp_rx_*_verify_dev over the UDP frames of the same lengths — its yardstick;
  echo    nsx_icmp_echo_reply_*_dev over the echo requests, every frame a hit;
  nat     nsx_nat_*_tcp_rewrite_dev over as many TCP frames of the same length, every frame a hit — its yardstick.
err, copy, rx and udp_rx: `--launches` back-to-back calls between two HIP events. echo and nat write in place, so a second
call would find other frames than the first: each call is timed alone between two events, with the type byte put back
(echo) before it, outside the events; nat's two rules turn one tuple into the other and back, so every call hits, and
the same strided one-byte write per frame runs before it (the TCP flags byte, to its own value), so that both legs
start from the same cache and queue state.
Before anything is timed the outputs are checked: every status is NSX_ICMP_SENT, every generated message passes
nsx_icmp_rx_*_verify_dev, every echo request verifies and is answered, the replies verify, every nat frame is
translated. There is no threshold: each leg is reported next to its yardstick, with the spread over the rounds. Bytes
moved = bytes read + bytes written (the copy: twice its bytes), the project's convention.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network-stack_amd")]


def config(tag, ipver, n, frame, rounds, launches, say, hip):
    import numpy as np
    import nsx
    import torch
    dev = torch.device("cuda", 0)
    iph, alen = (20, 4) if ipver == 4 else (40, 16)
    pay = frame - iph - 8
    assert frame % 4 == 0 and n % 64 == 0  # the build's slots are then dense; whole mask words

    def rnd(count, bits, dtype, seed):
        t = torch.empty(count * 8, dtype=torch.uint8, device=dev)
        nsx.fill_splitmix64_dev(t, seed)
        return (t.view(torch.int64) & ((1 << bits) - 1)).to(dtype)

    def addrs(seed):
        a = torch.empty(n * alen, dtype=torch.uint8, device=dev)
        nsx.fill_splitmix64_dev(a, seed)
        a.view(n, alen)[:, 0] = a.view(n, alen)[:, 0] % 223 + 1  # unicast: no frame is one to stay quiet about
        return a

    full = lambda m: bool((m[:n // 64] == -1).all())  # noqa: E731
    data = torch.empty(n * pay, dtype=torch.uint8, device=dev)
    nsx.fill_splitmix64_dev(data, 0x1C3F + pay)
    ip = {"src": addrs(1), "dst": addrs(2), "ident": rnd(n, 16, torch.int16, 3),
          "ttl": torch.full((n,), 64, dtype=torch.uint8, device=dev),
          "tclass": torch.zeros(n, dtype=torch.uint8, device=dev), "flow": torch.zeros(n, dtype=torch.int32, device=dev)}
    ports = {"src_port": rnd(n, 16, torch.int16, 5), "dst_port": rnd(n, 16, torch.int16, 6)}
    idx = torch.arange(n + 1, dtype=torch.int64, device=dev)
    offs = idx * frame
    udp = torch.empty(n * frame, dtype=torch.uint8, device=dev)
    (nsx.udp_tx_ipv4_build_dev if ipver == 4 else nsx.udp_tx_ipv6_build_dev)(ip, ports, data, idx * pay, udp, offs)
    udp_rx = nsx.udp_rx_ipv4_verify_dev if ipver == 4 else nsx.udp_rx_ipv6_verify_dev
    if not full(udp_rx(udp, offs)):
        raise SystemExit(f"{tag}: not every datagram verifies")
    del data
    # the echo requests: the same frames with protocol 1 / 58 and an ICMP header over the UDP one
    icmp = udp.clone()
    m = icmp.view(n, frame)
    rq = 8 if ipver == 4 else 128
    m[:, iph], m[:, iph + 1], m[:, iph + 2], m[:, iph + 3] = rq, 0, 0, 0
    if ipver == 4:
        m[:, 9], m[:, 10], m[:, 11] = 1, 0, 0
        nsx.ipv4_hdr_csum_dev(icmp, frame, n, mode=1)
        part = None
    else:
        m[:, 6] = 58
        part = nsx.pseudo_ipv6_partial_dev(ip["src"], ip["dst"], torch.full((n,), frame - 40, dtype=torch.int32, device=dev), 58)
    fld = ~nsx.fixed_dev(icmp[iph:], frame, frame - iph, n, partial=part).to(torch.int32) & 0xFFFF
    m[:, iph + 2], m[:, iph + 3] = (fld >> 8).to(torch.uint8), (fld & 0xFF).to(torch.uint8)
    rx_fn = nsx.icmp_rx_ipv4_verify_dev if ipver == 4 else nsx.icmp_rx_ipv6_verify_dev
    echo_fn = nsx.icmp_echo_reply_ipv4_dev if ipver == 4 else nsx.icmp_echo_reply_ipv6_dev
    mask = rx_fn(icmp, offs).clone()
    if not full(mask):
        raise SystemExit(f"{tag}: not every echo request verifies")
    rq_frames = icmp.clone()  # the verify leg's own copy: the echo leg writes in place
    hits = echo_fn(icmp, offs, mask, ttl=64).clone()
    if not (full(hits) and full(rx_fn(icmp, offs)) and bool((m[:, iph] == (0 if ipver == 4 else 129)).all())):
        raise SystemExit(f"{tag}: not every echo request was answered by a reply that verifies")
    m[:, iph] = rq  # requests again (the checksum is then the reply's: the echo pass does not look at it)
    # error generation over the UDP frames
    err_fn = nsx.icmp_err_ipv4_dev if ipver == 4 else nsx.icmp_err_ipv6_dev
    req = torch.full((n,), 11 if ipver == 4 else 3, dtype=torch.int32, device=dev)
    our = bytes([10, 0, 0, 1]) if ipver == 4 else bytes([0x20, 1, 0xd, 0xb8] + [0] * 11 + [1])
    work = torch.empty(nsx.icmp_err_work_bytes(n), dtype=torch.uint8, device=dev)
    res = err_fn(udp, offs, req, our, work=work)
    torch.cuda.synchronize()
    q = min(frame, nsx.ICMP_QUOTE[ipver])
    obytes = n * (nsx.ICMP_HDR[ipver] + q)
    if int(res["n_out"].item()) != n or int(res["out_off"][n].item()) != obytes or \
            not bool((res["status"][:n] == nsx.ICMP_SENT).all()) or not full(rx_fn(res["out"], res["out_off"][:n + 1])):
        raise SystemExit(f"{tag}: not every frame was answered by a message that verifies")
    err = lambda: err_fn(udp, offs, req, our, out=res, work=work)  # noqa: E731
    # the nat yardstick: n TCP frames of the same length with one tuple, two rules that turn it into another and back
    tcp_pay = frame - iph - 20
    one = lambda v, dt: torch.full((n,), v, dtype=dt, device=dev)  # noqa: E731
    fields = {"src_port": one(1234, torch.int16), "dst_port": one(80, torch.int16), "seq_num": rnd(n, 32, torch.int32, 7),
              "ack_num": rnd(n, 32, torch.int32, 8), "offset": one(5, torch.uint8), "control": one(0x10, torch.uint8),
              "window": one(512, torch.int16), "urgent_ptr": one(0, torch.int16)}
    a_src, a_dst = bytes(range(1, alen + 1)), bytes(range(101, alen + 101))
    tip = dict(ip, src=torch.tensor(list(a_src), dtype=torch.uint8, device=dev).repeat(n),
               dst=torch.tensor(list(a_dst), dtype=torch.uint8, device=dev).repeat(n))
    tdata = torch.zeros(n * tcp_pay, dtype=torch.uint8, device=dev)
    tcp = torch.empty(n * frame, dtype=torch.uint8, device=dev)
    toffs = offs
    (nsx.tx_ipv4_tcp_build_dev if ipver == 4 else nsx.tx_ipv6_tcp_build_dev)(tip, fields, tdata, idx * tcp_pay, tcp, toffs)
    ta = a_src + a_dst + (1234).to_bytes(2, "big") + (80).to_bytes(2, "big")
    tb = bytes(x ^ 0x55 for x in ta)
    match = np.frombuffer(ta + tb, np.uint8)
    slots = nsx.nat_table_slots(2)
    table = torch.from_numpy(nsx.nat_table_build_host(ipver, match, np.frombuffer(tb + ta, np.uint8), slots)).to(dev)
    tmask = (nsx.rx_ipv4_tcp_verify_dev if ipver == 4 else nsx.rx_ipv6_tcp_verify_dev)(tcp, toffs).clone()
    nat_fn = nsx.nat_ipv4_tcp_rewrite_dev if ipver == 4 else nsx.nat_ipv6_tcp_rewrite_dev
    thit = torch.empty_like(tmask)
    nat = lambda: nat_fn(tcp, toffs, tmask, table, slots, ttl_dec=0, hit=thit)  # noqa: E731
    nat()
    if not (full(tmask) and full(thit)):
        raise SystemExit(f"{tag}: not every TCP frame verifies and is translated")
    say(f"checked {tag}: {n} frames of {frame} B; {n} messages of {nsx.ICMP_HDR[ipver] + q} B ({obytes} B), every one "
        f"verifies; every echo request verifies, is answered, and the reply verifies; every nat frame is translated")
    dst = torch.empty(obytes, dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy():
        rc = hip.hipMemcpyAsync(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(res["out"].data_ptr()),
                                ctypes.c_size_t(obytes), 3, stream)  # hipMemcpyDeviceToDevice
        if rc != 0:
            raise SystemExit(f"hipMemcpyAsync: {rc}")

    mask2, umask, hit2 = torch.empty_like(mask), torch.empty_like(mask), torch.empty_like(mask)

    def reset():
        m[:, iph] = rq

    tm = tcp.view(n, frame)

    def nat_pre():  # the same strided one-byte write per frame as echo's reset (the ACK flag byte, to its own value)
        tm[:, iph + 13] = 0x10

    # (name, step, what runs before each timed call outside the events or None, bytes moved)
    legs = [("err", err, None, n * q + obytes), ("copy", copy, None, 2 * obytes),
            ("rx", lambda: rx_fn(rq_frames, offs, mask=mask2), None, n * frame),
            ("udp_rx", lambda: udp_rx(udp, offs, mask=umask), None, n * frame),
            ("echo", lambda: echo_fn(icmp, offs, mask, ttl=64, hit=hit2), reset, 0),
            ("nat", nat, nat_pre, 0)]
    t_end = time.perf_counter() + 0.5
    while time.perf_counter() < t_end:  # settle
        for _, step, pre, _ in legs:
            if pre:
                pre()
            step()
        torch.cuda.synchronize()
    times = {name: [] for name, _, _, _ in legs}
    for r in range(rounds):
        for name, step, pre, _ in (legs if r % 2 == 0 else legs[::-1]):
            for _ in range(2):
                if pre:
                    pre()
                step()
            if pre is None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    step()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / launches)
            else:
                ev = []
                for _ in range(launches):
                    pre()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step()
                    e1.record()
                    ev.append((e0, e1))
                torch.cuda.synchronize()
                times[name].append(statistics.median(a.elapsed_time(b) for a, b in ev))
    if not (full(hit2) and full(thit) and full(mask2)):
        raise SystemExit(f"{tag}: a timed call did not do what the checked one did")
    med = {k: statistics.median(x) for k, x in times.items()}
    for name, _, _, moved in legs:
        x = sorted(times[name])
        rate = f"  moved {moved / 1e6:.1f} MB  {moved / (med[name] * 1e-3) / 1e9:.1f} GB/s" if moved else \
            f"  {med[name] * 1e6 / n:.3f} ns per frame"
        say(f"ICMPAB {tag} {name:6s} median {med[name]:.5f} ms/call  min {x[0]:.5f} max {x[-1]:.5f} spread "
            f"{(x[-1] - x[0]) / med[name] * 100:.2f}%{rate}")
    for a, b in (("err", "copy"), ("rx", "udp_rx"), ("echo", "nat")):
        say(f"ICMPAB {tag} {a:6s} vs {b:6s}: time {med[a] / med[b]:.4f}")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icmp_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/icmp_ab.py measures on a GPU and found none")
    torch.cuda.set_device(0)
    import nsx
    hip = nsx.lib()  # dlsym through the product library's handle reaches the HIP runtime it is linked against
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n = max((1 << 20) // a.scale, 64) // 64 * 64
    for ipver, big in ((4, 1500), (6, 1520)):
        for frame in (big, 80):
            config(f"v{ipver}_{frame}B", ipver, n, frame, a.rounds, a.launches, say, hip)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# tools/icmp_ab.py on one MI355X, one process: {a.rounds} rounds x {a.launches} calls per leg, order "
                f"alternating\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
