"""Seeded random batches for the transmit pass, segmentation offload and receive coalescing: host arrays only (no
torch), shared by the GPU fuzz families of tests/test_gpu_zz_fuzz.py and the CPU self-check tests/test_fuzz_gen.py,
which keeps them from degenerating into trivial batches. Every generator is a pure function of its case number."""
import numpy as np

import _gro
import _gro_flow
import _tso
import _tx

# payload sizes around the copy kernel's row pair (2 x 64 chunks of 16 B = 2 KiB of destination) and jumbo frames
GRO_MSS = (1, 3, 7, 536, 1448, 1460, 1461, 2040, 2049, 4100, 8948, 8960)
TSO_MSS = (1, 2, 3, 7, 8, 536, 537, 1448, 1460, 1461, 2000, 8960, 65535)
GRO_BYTES, TSO_BYTES, TSO_SUPER_MAX = 1 << 20, 2 << 20, 70_000
NULLABLE = ("ident", "offset", "ttl", "tclass", "flow")
GRO_CASES, TSO_CASES, TX_CASES = 60, 40, 40  # the default seeds (NSX_FUZZ_SCALE multiplies them)


# ---------------------------------------------------------------- receive coalescing
def _payloads(rng, nf, mss):
    """One connection's payload profile."""
    profile = int(rng.integers(4))
    if profile == 0:  # every frame at one mss, the last 0..mss
        return [mss] * (nf - 1) + [int(rng.integers(0, mss + 1))]
    if profile == 1:  # tiny and empty payloads
        return rng.integers(0, 10, nf).tolist()
    if profile == 2:  # strictly falling
        return np.sort(rng.choice(max(mss, nf) + 1, nf, replace=False))[::-1].tolist()
    return [mss] * nf  # all equal


def _mutate(rng, f: bytes, ipver: int) -> bytes:
    """One of: a bit flipped in the TCP header, a bit flipped in the IP header, byte 12 replaced, the frame truncated;
    the checksums re-fixed wherever the frame is still long enough for its own header lengths."""
    iph = _tx.IPH[ipver]
    b = bytearray(f)
    kind = int(rng.integers(4))
    if kind == 0:
        b[iph + int(rng.integers(20))] ^= 1 << int(rng.integers(8))
    elif kind == 1:
        b[int(rng.integers(iph))] ^= 1 << int(rng.integers(8))
    elif kind == 2:
        b[iph + 12] = int(rng.integers(256))
    else:
        b = b[:int(rng.integers(len(b)))]
    ihl = (b[0] & 15) * 4 if ipver == 4 and b else iph
    if ihl >= 20 and len(b) >= ihl + 20:
        return _gro.refix(b, ipver)
    return bytes(b)


def gro_batch(case: int):
    """(ipver, buf, offsets, valid, untouched): 1-12 connections of 1-24 frames (tests/_gro.flow_case), each with its own
    payload profile, option set, closing flags and sequence / ident start, delivered connection by connection,
    round-robin or in a random interleave; ~8% of the frames mutated, ~4% of the valid bits clear, 0-3 lead bytes.
    untouched[i]: frame i is as the transmit pass made it."""
    rng = np.random.default_rng(0x6A0000 + case)
    ipver = 4 if case % 2 == 0 else 6
    conns, left = [], GRO_BYTES
    for _ in range(int(rng.integers(1, 13))):
        mss = int(rng.choice(GRO_MSS))
        pays = _payloads(rng, int(rng.integers(1, 25)), mss)
        key = int(rng.integers(4))
        opt = _tx.opt_bytes(rng, _gro.OPT_KEYS[key]) if key < 3 else b""
        size = np.cumsum([_tx.IPH[ipver] + 20 + len(opt) + p for p in pays])
        pays = pays[:int(np.searchsorted(size, left, side="right"))]  # the batch stays near 1 MiB
        if not pays:
            break
        left -= int(size[len(pays) - 1])
        seq0 = ((1 << 32) - int(rng.integers(0, 3 * mss + 1))) % (1 << 32) if rng.random() < 0.2 else None
        ident0 = 0xFFFF - int(rng.integers(0, 4)) if rng.random() < 0.2 else None
        c = _gro.flow_case(rng, ipver, pays, opt=opt, seq0=seq0, ident0=ident0)
        if rng.random() < 0.1:
            c.fields["control"][0] |= _gro.CWR
        if rng.random() < 1 / 3:
            c.fields["control"][-1] |= (_gro.FIN, _gro.PSH, _gro.FIN | _gro.PSH)[int(rng.integers(3))]
        conns.append(_gro.case_frames(c))
    delivery = int(rng.integers(3))
    if delivery == 0:
        frames = [f for c in conns for f in c]
    elif delivery == 1:
        frames, _ = _gro_flow.round_robin(conns)
    else:
        who = rng.permutation(np.repeat(np.arange(len(conns)), [len(c) for c in conns]))
        nxt = [0] * len(conns)
        frames = []
        for w in who:
            frames.append(conns[w][nxt[w]])
            nxt[w] += 1
    made = list(frames)
    for i in np.nonzero(rng.random(len(frames)) < 0.08)[0]:
        frames[i] = _mutate(rng, frames[i], ipver)
    untouched = np.array([a == b for a, b in zip(frames, made)], bool)
    valid = rng.random(len(frames)) >= 0.04
    buf, offs = _gro.pack(frames, lead=int(rng.integers(4)))
    return ipver, buf, offs, valid, untouched


# ---------------------------------------------------------------- transmit and segmentation offload
def _options(rng, n):
    """Per-entry option bytes from all of tests/_tx.OPT_SETS (a third of the entries without), or None: no option
    array at all."""
    if rng.random() < 0.25:
        return None
    keys = sorted(_tx.OPT_SETS)
    return [_tx.opt_bytes(rng, keys[int(rng.integers(len(keys)))]) if rng.random() < 2 / 3 else b"" for _ in range(n)]


def _slots(rng, packed):
    """The packed layout, or in a third of the cases the same slots with 0-60 bytes (multiples of 4) between them
    and 0-12 before the first."""
    if rng.random() >= 1 / 3:
        return packed
    n = packed.size - 1
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(np.diff(packed) + 4 * rng.integers(0, 16, n).astype(np.uint64))
    return off + np.uint64(4 * int(rng.integers(0, 4)))


def _nulls(rng):
    return tuple(k for k in NULLABLE if rng.random() < 0.3)


def tso_batch(case: int, buildable: bool = False):
    """(tests/_tso.Batch, out_off, null): 1-200 super-segments of 0..6 mss payload bytes (at most 70,000 each, 2 MiB in
    all), mss per super-segment or one for the batch; null: the optional arrays to pass as NULL. buildable: the same
    draw with the super-segments of mss 65535 cut to 65,000 payload bytes, so that every frame fits its IP length
    field (the host calls refuse a batch that holds one that does not)."""
    rng = np.random.default_rng(0x6B0000 + case)
    ipver = 4 if case % 2 == 0 else 6
    n = int(rng.integers(1, 201))
    mss = rng.choice(TSO_MSS, n) if rng.random() < 0.5 else np.full(n, int(rng.choice(TSO_MSS)))
    lens = np.minimum(rng.integers(0, 6 * mss + 1), TSO_SUPER_MAX)
    if buildable:
        lens = np.where(mss == 65535, np.minimum(lens, 65_000), lens)
    n = max(1, int(np.searchsorted(np.cumsum(lens), TSO_BYTES, side="right")))
    b = _tso.Batch(rng, ipver, lens[:n], mss[:n].astype(np.uint32), opts=_options(rng, n), lead=int(rng.integers(4)))
    return b, _slots(rng, b.off), _nulls(rng)


def tx_batch(case: int, buildable: bool = False):
    """A tests/_tx.Case of 1-400 frames with payloads of 0-9000 bytes (2 MiB in all), in a quarter of the cases a few
    of them with a TCP part around the most the IP length field carries, some past it; .out_off and .null as
    tso_batch returns them. buildable: the same draw with those frames cut to 65,000 payload bytes."""
    rng = np.random.default_rng(0x6C0000 + case)
    ipver = 4 if case % 2 == 0 else 6
    n = int(rng.integers(1, 401))
    hi = int(rng.choice([40, 1500, 9000]))
    lens = rng.integers(0, hi + 1, n)
    if rng.random() < 0.25:
        at = rng.integers(0, n, int(rng.integers(1, 4)))
        lens[at] = _tx.WIRE_MAX[ipver] - 20 - rng.integers(-30, 60, at.size)
        if buildable:
            lens[at] = 65_000
    n = max(1, int(np.searchsorted(np.cumsum(lens), TSO_BYTES, side="right")))
    c = _tx.Case(rng, ipver, lens[:n], opts=_options(rng, n), lead=int(rng.integers(4)))
    c.out_off, c.null = _slots(rng, c.packed()), _nulls(rng)
    return c


def ip_overrides(null):
    """tests/_tx.expected's keyword arguments for the IP fields passed as NULL (ident 0, ttl 64, tclass 0, flow 0)."""
    return {k: v for k, v in (("ident", 0), ("ttl", 64), ("tclass", 0), ("flow", 0)) if k in null}
