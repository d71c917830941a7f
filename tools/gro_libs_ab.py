#!/usr/bin/env python3
"""nsx_gro_* of two builds of the library timed in one process: has the call moved against another build?

    python tools/gro_libs_ab.py --other-lib PATH/libnsx_csum.so [--rounds 12] [--launches 10] [--ipver 0|4|6]

Runs of tools/gro_ab.py in separate processes differ in their gro leg by a percent or two for one and the same library,
far more than the spread inside a process, so two libraries are told apart here: the binding is loaded a second time
over the other build (for instance the parent commit's, built into another directory), and the mss1460 shape of
tools/gro_ab.py (23,832 runs of 44 frames of 1460 B) is timed in interleaved rounds whose order alternates, legs
other, this, other2, this2 between two tso legs of this tree's library, `--launches` back-to-back calls bracketed by
HIP events. The other build may predate nsx_gro_flow_*.
"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "network-stack_amd"), os.path.join(ROOT, "tools")]


def load_other(path):
    """The binding once more, under another module name, over the library at `path`."""
    spec = importlib.util.spec_from_file_location("nsx_other", os.path.join(ROOT, "network-stack_amd", "nsx",
                                                                             "__init__.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.LIB_PATH = os.path.abspath(path)
    m.lib()
    return m


def shape(other, ipver, rounds, launches, nsup=23832, cnt=44, mss=1460):
    import nsx
    import torch
    from gro_ab import wrap
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0x770 + mss + ipver)
    ri = lambda hi, n, dt: torch.randint(0, hi, (n,), generator=g, device=dev, dtype=torch.int64).to(dt)  # noqa: E731
    iph, alen = (20, 4) if ipver == 4 else (40, 16)
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
    sdoff = torch.arange(nsup + 1, dtype=torch.int64, device=dev) * (cnt * mss)
    data = torch.empty(nsup * cnt * mss, dtype=torch.uint8, device=dev)
    nsx.fill_splitmix64_dev(data, 0x770)
    dmss = torch.full((nsup,), mss, dtype=torch.int32, device=dev)
    first = torch.arange(nsup + 1, dtype=torch.int64, device=dev) * cnt
    fseg = (torch.arange(nf, dtype=torch.int64, device=dev) // cnt).to(torch.int32)
    out_off = torch.arange(nf + 1, dtype=torch.int64, device=dev) * (mss + iph + 20)
    frames = torch.empty(nf * (mss + iph + 20), dtype=torch.uint8, device=dev)
    v = "ipv4" if ipver == 4 else "ipv6"
    tso_fn, gro_this, gro_other = (getattr(nsx, f"tso_{v}_tcp_build_dev"), getattr(nsx, f"gro_{v}_tcp_dev"),
                                   getattr(other, f"gro_{v}_tcp_dev"))

    def tso():
        tso_fn(ip, sup, data, sdoff, dmss, first, fseg, frames, out_off)

    tso()
    mask = getattr(nsx, f"rx_{v}_tcp_verify_dev")(frames, out_off)
    work = torch.empty(nsx.gro_work_bytes(nf), dtype=torch.uint8, device=dev)
    out = gro_this(frames, out_off, mask, work=work)
    torch.cuda.synchronize()
    if int(out["n_super"].item()) != nsup or not torch.equal(out["data"][:data.numel()], data):
        raise SystemExit("receive coalescing did not give back the batch the frames were cut from")

    def this():
        gro_this(frames, out_off, mask, out=out, work=work)

    def that():
        gro_other(frames, out_off, mask, out=out, work=work)

    legs = [("tso", tso), ("other", that), ("this", this), ("other2", that), ("this2", this), ("tso2", tso)]
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
    tag = f"mss1460_v{ipver}"
    for k, x in res.items():
        print(f"GROLIBS {tag} {k:6s} median {med[k]:.5f} ms/call  min {min(x):.5f} max {max(x):.5f}", flush=True)
    o, t = (med["other"] + med["other2"]) / 2, (med["this"] + med["this2"]) / 2
    print(f"GROLIBS {tag}: this / other {t / o:.4f}; spread between the two legs of the other library "
          f"{abs(med['other'] - med['other2']) / o * 100:.2f}%, of this one "
          f"{abs(med['this'] - med['this2']) / t * 100:.2f}%, of tso {abs(med['tso'] - med['tso2']) / med['tso'] * 100:.2f}%", flush=True)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", required=True, help="another build of libnsx_csum.so")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--ipver", type=int, default=0, choices=[0, 4, 6])
    a = ap.parse_args()
    other = load_other(a.other_lib)
    torch.cuda.set_device(0)
    for ipver in (4, 6):
        if a.ipver in (0, ipver):
            shape(other, ipver, a.rounds, a.launches)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
