"""IPv4 fragmentation and reassembly (nsx_frag_ipv4_dev, nsx_reasm_ipv4_dev) restated in numpy and plain Python from the
contract comment of include/nsx_csum.h alone: the frame map of the host helpers, the device rule frame by frame with
the RFC 1624 checksum update, the member test, the key, the order, cont(p), the runs and every output array — without
looking at the library. tests/test_frag_abi.py holds it to its own round trip and to the receive verifies of
tests/_udp.py and tests/_rx.py. Input frames come from tests/_udp.py and tests/_tx.py. No torch and no GPU at import."""
import numpy as np

import _tx
import _udp

PASS, CUT, DF, BAD = 0, 1, 2, 3
NONE = 0xFFFFFFFF
NO_KEY = 0xFFFFFFFF
LEN_CAP = 1 << 30


# ------------------------------------------------------------------ the frame map
def per_of(mtu: int) -> int:
    return (mtu - 20) & ~7


def slots_of(length: int, mtu: int) -> int:
    return 1 if length <= mtu else -(-(length - 20) // per_of(mtu))


def count(offsets, mtu):
    """nsx_frag_count_host restated: frag_first (n + 1), or None where the call refuses."""
    offsets = [int(x) for x in offsets]
    n = len(offsets) - 1
    if n >= 1 << 32:
        return None
    first = [0]
    for i in range(n):
        L = offsets[i + 1] - offsets[i]
        if L < 0 or L >= LEN_CAP or int(mtu[i]) < 28:
            return None
        first.append(first[-1] + slots_of(L, int(mtu[i])))
    return np.array(first, np.uint64)


def layout(offsets, mtu, first):
    """nsx_frag_layout_host restated: (frag_src u32, out_off u64), or None where the call refuses."""
    want = count(offsets, mtu)
    if want is None or not np.array_equal(want, np.asarray(first, np.uint64)):
        return None
    src, off = [], [0]
    for i in range(len(offsets) - 1):
        L, m = int(offsets[i + 1]) - int(offsets[i]), int(mtu[i])
        for j in range(slots_of(L, m)):
            src.append(i)
            off.append(off[-1] + (L if L <= m else 20 + min(per_of(m), L - 20 - j * per_of(m))))
    return np.array(src, np.uint32), np.array(off, np.uint64)


# ------------------------------------------------------------------ fragmentation
def fold(x: int) -> int:
    return 0 if x == 0 else 1 + (x - 1) % 0xFFFF


def be16(b, k) -> int:
    return (int(b[k]) << 8) | int(b[k + 1])


def status_of(f: bytes, mtu: int) -> int:
    L = len(f)
    if mtu < 28:
        return BAD
    if L <= mtu:
        return PASS
    o = be16(f, 6) & 0x1FFF
    if f[0] != 0x45 or be16(f, 2) != L or o * 8 + L - 20 > 65535:
        return BAD
    return DF if f[6] & 0x40 else CUT


def cut(f: bytes, mtu: int):
    """The fragments of a frame whose status is CUT."""
    per, pay = per_of(mtu), len(f) - 20
    f16, hc = be16(f, 6), be16(f, 10)
    out = []
    for j in range(-(-pay // per)):
        piece = f[20 + j * per:20 + min((j + 1) * per, pay)]
        last = (j + 1) * per >= pay
        n1 = 20 + len(piece)
        n3 = (f16 & 0xC000) | ((f16 & 0x2000) if last else 0x2000) | ((f16 & 0x1FFF) + j * per // 8)
        nc = ~fold((~hc & 0xFFFF) + (~len(f) & 0xFFFF) + n1 + (~f16 & 0xFFFF) + n3) & 0xFFFF
        h = bytearray(f[:20])
        h[2:4], h[6:8], h[10:12] = n1.to_bytes(2, "big"), n3.to_bytes(2, "big"), nc.to_bytes(2, "big")
        out.append(bytes(h) + piece)
    return out


def frag(buf, offsets, mtu, fill=0):
    """(out, out_off, frag_first, frag_src, status) of the device call over frames buf[offsets[i], offsets[i+1]) with
    the host helpers' frame map; out is out_off[-1] bytes."""
    buf = np.asarray(buf, np.uint8)
    first = count(offsets, mtu)
    src, off = layout(offsets, mtu, first)
    out = np.full(int(off[-1]), fill, np.uint8)
    status = np.zeros(len(offsets) - 1, np.uint8)
    for i in range(len(offsets) - 1):
        f = buf[int(offsets[i]):int(offsets[i + 1])].tobytes()
        st = status[i] = status_of(f, int(mtu[i]))
        t0, t1 = int(first[i]), int(first[i + 1])
        if st == PASS:
            pieces = [f]
        elif st == CUT:
            pieces = cut(f, int(mtu[i]))
        else:
            pieces = [bytes(int(off[t + 1]) - int(off[t])) for t in range(t0, t1)]
        assert len(pieces) == t1 - t0
        for t, p in zip(range(t0, t1), pieces):
            assert len(p) == int(off[t + 1]) - int(off[t])
            out[int(off[t]):int(off[t + 1])] = np.frombuffer(p, np.uint8)
    return out, off, first, src, status


def frag_frames(frames, mtu):
    """The output slots of `frag` as a list of bytes, with the statuses."""
    buf, offs = _udp.concat([np.frombuffer(f, np.uint8) for f in frames])
    mtu = np.broadcast_to(np.asarray(mtu, np.uint32), len(frames))
    out, off, _, _, status = frag(buf, offs, mtu)
    return [out[int(off[t]):int(off[t + 1])].tobytes() for t in range(off.size - 1)], status


# ------------------------------------------------------------------ reassembly
def member(f: bytes):
    """(offset field, payload bytes, MF) of a member, else None."""
    L = len(f)
    if L < 21 or f[0] != 0x45 or be16(f, 2) != L or _udp.raw(np.frombuffer(f[:20], np.uint8)) != 0xFFFF:
        return None
    f16 = be16(f, 6)
    o, mf, pay = f16 & 0x1FFF, bool(f16 & 0x2000), L - 20
    if not (mf or o) or pay < 1 or (mf and pay % 8) or o * 8 + pay > 65515:
        return None
    return o, pay, mf


def key(f: bytes) -> int:
    if member(f) is None:
        return NO_KEY
    h = 0x811C9DC5
    for w in (int.from_bytes(f[12:16], "little"), int.from_bytes(f[16:20], "little"), f[4] | f[5] << 8 | f[9] << 16):
        h = ((h ^ w) * 0x01000193) % (1 << 32)
    return h


def order_of(frames):
    mem = [member(f) for f in frames]
    off = np.array([m[0] if m else 0 for m in mem], np.uint32)
    keys = np.array([key(f) for f in frames], np.uint32)
    o1 = np.argsort(off, kind="stable")
    od = o1[np.argsort(keys[o1], kind="stable")]
    assert np.array_equal(od, np.lexsort((np.arange(len(frames)), off, keys)))
    return od.astype(np.uint32), mem


def reasm(buf, offsets) -> dict:
    """The outputs of the device call, exactly sized: per-datagram arrays of n_out entries, out_off of n_out + 1, out
    of its packed length, frame_seg and order of n, is_frag of ceil(n/64) words."""
    buf = np.asarray(buf, np.uint8)
    offsets = np.asarray(offsets, np.uint64)
    n = offsets.size - 1
    frames = [buf[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(n)]
    od, mem = order_of(frames) if n else (np.zeros(0, np.uint32), [])
    bits = np.zeros((n + 63) // 64 * 64, np.uint8)
    bits[:n] = [m is not None for m in mem]
    res = dict(order=od, is_frag=np.packbits(bits, bitorder="little").view(np.uint64),
               frame_seg=np.full(n, NONE, np.uint32))

    def cont(p):
        if p == 0:
            return False
        a, b = int(od[p - 1]), int(od[p])
        ma, mb, fa, fb = mem[a], mem[b], frames[a], frames[b]
        if ma is None or mb is None:
            return False
        if fa[12:20] != fb[12:20] or fa[4:6] != fb[4:6] or fa[9] != fb[9]:
            return False
        return ma[2] and mb[0] * 8 == ma[0] * 8 + ma[1]

    out, out_off, first_pos, frag_cnt = [], [0], [], []
    p = 0
    while p < n:
        q = p
        while q + 1 < n and cont(q + 1):
            q += 1
        mh, ml = mem[int(od[p])], mem[int(od[q])]
        if mh is not None and ml is not None and mh[0] == 0 and not ml[2]:
            s = len(first_pos)
            dlen = 20 + ml[0] * 8 + ml[1]
            d = np.zeros(dlen, np.uint8)
            h = bytearray(frames[int(od[p])][:20])
            h[2:4] = dlen.to_bytes(2, "big")
            h[6], h[7] = h[6] & 0xC0, 0
            h[10:12] = b"\0\0"
            h[10:12] = (~_udp.raw(np.frombuffer(bytes(h), np.uint8)) & 0xFFFF).to_bytes(2, "big")
            d[:20] = np.frombuffer(bytes(h), np.uint8)
            for r in range(p, q + 1):
                i = int(od[r])
                o, pay, _ = mem[i]
                d[20 + o * 8:20 + o * 8 + pay] = np.frombuffer(frames[i][20:], np.uint8)
                res["frame_seg"][i] = s
            out.append(d)
            out_off.append(out_off[-1] + dlen)
            first_pos.append(p)
            frag_cnt.append(q - p + 1)
        p = q + 1
    res.update(n_out=len(first_pos), out=np.concatenate(out) if out else np.zeros(0, np.uint8),
               out_off=np.array(out_off, np.uint64), first_pos=np.array(first_pos, np.uint64),
               frag_cnt=np.array(frag_cnt, np.uint32))
    return res


def datagrams(res):
    """The reassembled datagrams of a `reasm` result as a list of bytes."""
    o = res["out_off"]
    return [res["out"][int(o[s]):int(o[s + 1])].tobytes() for s in range(int(res["n_out"]))]


# ------------------------------------------------------------------ frames to test with
def clear_df(f: bytes) -> bytes:
    """The IPv4 frame with DF cleared (the transmit passes set it) and the header checksum redone."""
    g = bytearray(f)
    g[6] &= 0xBF
    return _udp.fix4(np.frombuffer(bytes(g), np.uint8)).tobytes()


def udp_frames(rng, pays, df=False):
    """IPv4/UDP datagrams as the UDP transmit pass builds them (tests/_udp.py), DF cleared unless asked for."""
    c = _udp.Case(rng, 4, [int(p) for p in pays])
    fr, _ = _udp.frames(c)
    return [f.tobytes() if df else clear_df(f.tobytes()) for f in fr]


def tcp_frames(rng, pays, df=False):
    """IPv4/TCP datagrams as the TCP transmit pass builds them (tests/_tx.py), DF cleared unless asked for."""
    c = _tx.Case(rng, 4, [int(p) for p in pays])
    buf, _ = _tx.expected(c, c.packed())
    off = c.packed()
    fr = [buf[int(off[i]):int(off[i]) + int(c.flen[i])].tobytes() for i in range(c.n)]
    return fr if df else [clear_df(f) for f in fr]


def with_header(f: bytes, **kw) -> bytes:
    """The frame with header fields replaced — ident, mf, off (the 13-bit field), src, dst, proto, ttl — and the header
    checksum redone."""
    g = bytearray(f)
    if "ident" in kw:
        g[4:6] = int(kw["ident"]).to_bytes(2, "big")
    f16 = be16(g, 6)
    if "mf" in kw:
        f16 = (f16 & ~0x2000) | (0x2000 if kw["mf"] else 0)
    if "off" in kw:
        f16 = (f16 & ~0x1FFF) | int(kw["off"])
    g[6:8] = f16.to_bytes(2, "big")
    for k, at in (("src", 12), ("dst", 16)):
        if k in kw:
            g[at:at + 4] = bytes(kw[k])
    if "proto" in kw:
        g[9] = kw["proto"]
    if "ttl" in kw:
        g[8] = kw["ttl"]
    return _udp.fix4(np.frombuffer(bytes(g), np.uint8)).tobytes()


def pack(frames, lead: int = 0, tail: int = 3):
    """Frames packed back to back behind `lead` bytes of 0xEE (and `tail` after): (buf, offsets)."""
    lens = [len(f) for f in frames]
    offs = np.zeros(len(frames) + 1, np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64) if lens else 0
    offs += np.uint64(lead)
    buf = np.frombuffer(bytes([0xEE]) * lead + b"".join(frames) + bytes([0xEE]) * tail, np.uint8).copy()
    return buf, offs
