"""Seeded random batches for the fragmentation / reassembly fuzz (tests/test_gpu_frag_fuzz.py); tests/test_frag_gen.py
holds every seed to a floor of what it must contain, so no seed is vacuous. No torch and no GPU at import."""
import numpy as np

import _frag as F

SEEDS = range(20)
MTUS = (28, 68, 576, 1500, 4100)


def tune(rng):
    """Random launch overrides of nsx_frag_tune.h (None = the product call)."""
    if rng.integers(4) == 0:
        return None
    return dict(blocks_per_cu=int(rng.integers(0, 9)), run_segs=int(rng.choice([0, 1, 16, 17, 64, 4096])),
                rows=int(rng.choice([0, 1, 2, 16, 64])))


def frag_batch(seed):
    """(buf, offsets, mtu) for nsx_frag_ipv4_dev: frames that fit, frames to cut (some of them fragments already),
    DF frames and bad ones, each with an mtu of its own, behind 0..15 lead bytes."""
    rng = np.random.default_rng([0xF6C0, seed])
    frames, mtu = [], []
    for _ in range(int(rng.integers(40, 120))):
        m = int(rng.choice(MTUS))
        kind = rng.choice(["fit", "cut", "cut", "recut", "df", "bad", "tcp"])
        hi = {28: 200, 68: 600}.get(m, 3 * m)
        if kind == "fit":
            f = F.udp_frames(rng, [int(rng.integers(0, max(m - 27, 1)))])[0] if m > 28 else \
                rng.integers(0, 256, int(rng.integers(0, 29)), dtype=np.uint8).tobytes()
        elif kind == "tcp":
            f = F.tcp_frames(rng, [int(rng.integers(0, hi))])[0]
        else:
            f = F.udp_frames(rng, [int(rng.integers(m, hi + m))], df=kind == "df")[0]
            if kind == "recut":
                f = F.cut(f, 20 + max(8, ((len(f) - 20) // 2) & ~7))[int(rng.integers(2))]
            if kind == "bad":
                g = bytearray(f)
                how = int(rng.integers(4))
                if how == 0:
                    g[0] = 0x46
                elif how == 1:
                    g[0] = 0x65
                elif how == 2:
                    g[2:4] = (len(g) + 1).to_bytes(2, "big")
                else:
                    g[6:8] = (0x1FFF).to_bytes(2, "big")
                f = bytes(g)
        frames.append(f)
        mtu.append(m)
    # one of each status, whatever was drawn
    frames += [F.udp_frames(rng, [10])[0], F.udp_frames(rng, [3000])[0], F.udp_frames(rng, [3000], df=True)[0],
               rng.integers(0, 256, 2000, dtype=np.uint8).tobytes()]
    mtu += [1500, 1500, 1500, 576]
    buf, offs = F.pack(frames, lead=int(rng.integers(16)))
    return buf, offs, np.array(mtu, np.uint32)


def reasm_batch(seed):
    """(buf, offsets) for nsx_reasm_ipv4_dev: datagrams cut at random mtus (some fragments cut again), shuffled, with
    fragments lost and duplicated, non-fragments, wrong header checksums and same-ident datagrams among them."""
    rng = np.random.default_rng([0xF6C1, seed])
    frames = []
    same = (rng.integers(0, 256, 8, dtype=np.uint8).tobytes(), int(rng.integers(1 << 16)))
    for r in range(int(rng.integers(30, 90))):
        m = int(rng.choice(MTUS[:4]))
        hi = {28: 120, 68: 500}.get(m, 4 * m)
        f = F.udp_frames(rng, [int(rng.integers(max(m - 27, 1), hi))])[0]
        if rng.integers(8) == 0:  # RFC 4963: the same (src, dst, ident, protocol) as another datagram of the batch
            f = F.with_header(f, src=same[0][:4], dst=same[0][4:], ident=same[1])
        fr = F.cut(f, m)
        if len(fr) >= 2 and rng.integers(4) == 0 and len(fr[0]) > 64:
            fr = F.cut(fr[0], 20 + (((len(fr[0]) - 20) // 2) & ~7)) + fr[1:]
        fate = rng.integers(6)
        if fate == 0:
            del fr[int(rng.integers(len(fr)))]
        elif fate == 1:
            fr.append(fr[int(rng.integers(len(fr)))])
        elif fate == 2:
            k = int(rng.integers(len(fr)))
            g = bytearray(fr[k])
            g[int(rng.choice([1, 4, 8, 10, 13, 18]))] ^= 1 << int(rng.integers(8))
            fr[k] = bytes(g)
        frames += fr
        if rng.integers(3) == 0:
            frames.append(F.udp_frames(rng, [int(rng.integers(0, 200))])[0])
        if rng.integers(10) == 0:
            frames.append(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8).tobytes())
    # a complete datagram of five fragments, a leftover and a non-member, whatever was drawn
    f = F.udp_frames(rng, [600])[0]
    frames += F.cut(f, 148) + F.cut(F.udp_frames(rng, [600])[0], 148)[1:] + [F.udp_frames(rng, [20])[0]]
    rng.shuffle(frames)
    return F.pack(frames, lead=int(rng.integers(16)))
