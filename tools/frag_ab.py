#!/usr/bin/env python3
"""Same-process timing of IPv4 fragmentation and reassembly against a plain device-to-device copy, on one MI355X.

    python tools/frag_ab.py [--rounds 10] [--launches 5] [--scale 1] [--out profiles/frag_ab.txt]

Two sizes: 1 M UDP datagrams of 1500 B cut to mtu 576 (three fragments each), and 64 K datagrams of 8 KiB cut to mtu
1500 (six each); --scale divides both counts (rehearsals). The datagrams are built on the device by
nsx_udp_tx_ipv4_build_dev with random addresses, DF cleared with the header checksum updated. Per size four legs run in
interleaved rounds whose order alternates, `--launches` back-to-back calls between two HIP events:
  frag        nsx_frag_ipv4_dev over the datagrams (one launch);
  copy_frag   hipMemcpyAsync, device to device, of the bytes frag writes;
  reasm       nsx_reasm_ipv4_dev over the fragments as frag wrote them (key pass, two radix sorts, the run passes, copy);
  copy_reasm  hipMemcpyAsync of the bytes reasm writes.
The copy is the yardstick, measured in the same run; there is no threshold. Before anything is timed the outputs are
checked: every status is NSX_FRAG_CUT, every fragment's header sum is 0xFFFF (a sample), and the reassembled datagrams
all pass nsx_udp_rx_ipv4_verify_dev and are as many as the batch, less the few that lose to a 32-bit key collision (the
count is printed). Bytes moved = bytes read + bytes written (the copy: twice its bytes), the project's convention.
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network-stack_amd")]


def config(tag, n, frame, mtu, rounds, launches, say, hip):
    import numpy as np
    import nsx
    import torch
    dev = torch.device("cuda", 0)
    pay = frame - 28
    assert frame % 4 == 0  # the build's slots are then dense

    def rnd(count, bits, dtype, seed):
        t = torch.empty(count * 8, dtype=torch.uint8, device=dev)
        nsx.fill_splitmix64_dev(t, seed)
        return (t.view(torch.int64) & ((1 << bits) - 1)).to(dtype)

    data = torch.empty(n * pay, dtype=torch.uint8, device=dev)
    nsx.fill_splitmix64_dev(data, 0xF4A6 + pay)
    ip = {"src": rnd(n, 32, torch.int32, 1).view(torch.uint8), "dst": rnd(n, 32, torch.int32, 2).view(torch.uint8),
          "ident": rnd(n, 16, torch.int16, 3), "ttl": rnd(n, 8, torch.uint8, 4),
          "tclass": torch.zeros(n, dtype=torch.uint8, device=dev), "flow": torch.zeros(n, dtype=torch.int32, device=dev)}
    ports = {"src_port": rnd(n, 16, torch.int16, 5), "dst_port": rnd(n, 16, torch.int16, 6)}
    idx = torch.arange(n + 1, dtype=torch.int64, device=dev)
    offs = idx * frame
    frames = torch.empty(n * frame, dtype=torch.uint8, device=dev)
    nsx.udp_tx_ipv4_build_dev(ip, ports, data, idx * pay, frames, offs)
    # DF cleared, RFC 1624 eqn. 3 over word 3 (0x4000 -> 0)
    m = frames.view(n, frame)
    cs = (m[:, 10].to(torch.int64) << 8) | m[:, 11].to(torch.int64)
    x = (~cs & 0xFFFF) + 0xBFFF
    cs = ~(1 + (x - 1) % 0xFFFF) & 0xFFFF
    m[:, 6] = 0
    m[:, 10] = (cs >> 8).to(torch.uint8)
    m[:, 11] = (cs & 0xFF).to(torch.uint8)
    del data, m, cs, x
    if not bool((nsx.udp_rx_ipv4_verify_dev(frames, offs)[:n // 64] == -1).all()):
        raise SystemExit(f"{tag}: not every datagram verifies")
    h_offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(frame)
    h_mtu = np.full(n, mtu, np.uint32)
    first = nsx.frag_count_host(h_offs, h_mtu)
    src, out_off = nsx.frag_layout_host(h_offs, h_mtu, first)
    nf, fbytes = src.size, int(out_off[-1])
    d = lambda a, dt: torch.from_numpy(a.view(dt)).to(dev)  # noqa: E731
    d_mtu, d_first, d_src, d_out_off = d(h_mtu, np.int32), d(first, np.int64), d(src, np.int32), d(out_off, np.int64)
    frags = torch.empty(fbytes, dtype=torch.uint8, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    frag = lambda: nsx.frag_ipv4_dev(frames, offs, d_mtu, d_first, d_src, frags, d_out_off, status=status)  # noqa: E731
    frag()
    torch.cuda.synchronize()
    if not bool((status == nsx.FRAG_CUT).all()):
        raise SystemExit(f"{tag}: not every datagram was cut")
    for t in range(0, nf, max(nf // 64, 1)):
        h = frags[int(out_off[t]):int(out_off[t]) + 20].to(torch.int64)
        s = int(((h[0::2] << 8) | h[1::2]).sum().item())
        while s >> 16:
            s = (s & 0xFFFF) + (s >> 16)
        if s != 0xFFFF:
            raise SystemExit(f"{tag}: the header of fragment {t} does not verify")
    work = torch.empty(nsx.reasm_work_bytes(nf), dtype=torch.uint8, device=dev)
    res = nsx.reasm_ipv4_dev(frags, d_out_off, work=work)
    torch.cuda.synchronize()
    n_out = int(res["n_out"].item())
    rbytes = int(res["out_off"][n_out].item())
    mask = nsx.udp_rx_ipv4_verify_dev(res["out"], res["out_off"][:n_out + 1])
    bits = int(sum(bin(int(w) & 0xFFFFFFFFFFFFFFFF).count("1") for w in mask[:(n_out + 63) // 64].cpu().tolist()))
    if bits != n_out or n_out > n or n_out < n - max(n // 500, 4) or rbytes != n_out * frame:
        raise SystemExit(f"{tag}: {n_out} datagrams of {n} reassembled, {bits} verify, {rbytes} B")
    order = res.pop("order")
    reasm = lambda: nsx.reasm_ipv4_dev(frags, d_out_off, out=res, order=order, work=work)  # noqa: E731
    say(f"checked {tag}: {n} datagrams of {frame} B -> {nf} fragments at mtu {mtu} ({fbytes} B) -> {n_out} datagrams "
        f"({n - n_out} lost to key collisions), every one verifies")
    dst = torch.empty(max(fbytes, rbytes), dtype=torch.uint8, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy(nbytes):
        def step():
            rc = hip.hipMemcpyAsync(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(frags.data_ptr()),
                                    ctypes.c_size_t(nbytes), 3, stream)  # hipMemcpyDeviceToDevice
            if rc != 0:
                raise SystemExit(f"hipMemcpyAsync: {rc}")
        return step

    legs = [("frag", frag), ("copy_frag", copy(fbytes)), ("reasm", reasm), ("copy_reasm", copy(rbytes))]
    moved = {"frag": n * frame + fbytes, "copy_frag": 2 * fbytes, "reasm": fbytes + rbytes, "copy_reasm": 2 * rbytes}
    t_end = time.perf_counter() + 0.5
    while time.perf_counter() < t_end:  # settle
        for _, step in legs:
            step()
        torch.cuda.synchronize()
    times = {name: [] for name, _ in legs}
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
            times[name].append(e0.elapsed_time(e1) / launches)
    med = {k: statistics.median(x) for k, x in times.items()}
    for name, _ in legs:
        x = sorted(times[name])
        say(f"FRAGAB {tag} {name:10s} median {med[name]:.5f} ms/call  min {x[0]:.5f} max {x[-1]:.5f} spread "
            f"{(x[-1] - x[0]) / med[name] * 100:.2f}%  moved {moved[name] / 1e6:.1f} MB  "
            f"{moved[name] / (med[name] * 1e-3) / 1e9:.1f} GB/s")
    for a, b in (("frag", "copy_frag"), ("reasm", "copy_reasm")):
        say(f"FRAGAB {tag} {a:10s} vs {b:10s}: time {med[a] / med[b]:.4f}  rate "
            f"{(moved[a] / med[a]) / (moved[b] / med[b]):.4f}")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frag_ab.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/frag_ab.py measures on a GPU and found none")
    torch.cuda.set_device(0)
    import nsx
    hip = nsx.lib()  # dlsym through the product library's handle reaches the HIP runtime it is linked against
    hip.hipMemcpyAsync.restype = ctypes.c_int
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for tag, n, frame, mtu in (("1500B_mtu576", 1 << 20, 1500, 576), ("8KiB_mtu1500", 1 << 16, 8192, 1500)):
        config(tag, max(n // a.scale, 64) // 64 * 64, frame, mtu, a.rounds, a.launches, say, hip)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# tools/frag_ab.py on one MI355X, one process: {a.rounds} rounds x {a.launches} calls per leg, order "
                f"alternating\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
