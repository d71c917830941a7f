"""TCP receive coalescing (nsx_gro_ipv4_tcp_dev / nsx_gro_ipv6_tcp_dev) restated in numpy and plain Python: the rules
of include/nsx_csum.h — member, same(i, i-1), join(i) with its three-frame window, and every output array — frame by
frame, without looking at the library. tests/test_gro_abi.py holds it to segmentation offload's expansion
(tests/_tso.py): coalescing the frames of a super-segment batch gives the batch back."""
import numpy as np

import _tso
import _tx

FIN, SYN, RST, PSH, ACK, URG, ECE, CWR = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
NONE = 0xFFFFFFFF
PER_SUPER = (("ident", np.uint16), ("ttl", np.uint8), ("tclass", np.uint8), ("flow", np.uint32),
             ("src_port", np.uint16), ("dst_port", np.uint16), ("seq_num", np.uint32), ("ack_num", np.uint32),
             ("offset", np.uint8), ("control", np.uint8), ("window", np.uint16), ("urgent_ptr", np.uint16),
             ("mss", np.uint32), ("first_frame", np.uint64), ("frame_cnt", np.uint32))


def valid_bits(valid, n):
    """The receive pass's mask (uint64 words) or a boolean array → n booleans."""
    valid = np.asarray(valid)
    if valid.dtype == np.bool_:
        return valid[:n].copy()
    return np.unpackbits(np.ascontiguousarray(valid, np.uint64).view(np.uint8), bitorder="little")[:n].astype(bool)


def parse(f: bytes, ipver: int):
    """The member's view of one frame, or None when it is not well-formed as the receive pass defines or its data
    offset does not fit (5 <= doff, doff*4 <= segment length)."""
    L = len(f)
    if ipver == 4:
        if L < 20 or f[0] >> 4 != 4:
            return None
        ihl = (f[0] & 15) * 4
        if ihl < 20 or ihl > L or int.from_bytes(f[2:4], "big") != L:
            return None
        if f[6] & 0x20 or (f[6] & 0x1F) or f[7] or f[9] != 6 or L - ihl < 20:
            return None
        ip = dict(src=f[12:16], dst=f[16:20], ttl=f[8], ihl=ihl, tos=f[1], b67=f[6:8],
                  ident=int.from_bytes(f[4:6], "big"), tclass=f[1], flow=0)
    else:
        if L < 40 or f[0] >> 4 != 6 or 40 + int.from_bytes(f[4:6], "big") != L or f[6] != 6 or L - 40 < 20:
            return None
        ihl = 40
        w = int.from_bytes(f[0:4], "big")
        ip = dict(src=f[8:24], dst=f[24:40], ttl=f[7], vcf=f[0:4], ident=0, tclass=(w >> 20) & 0xFF, flow=w & 0xFFFFF)
    t = f[ihl:]
    doff = t[12] >> 4
    if doff < 5 or doff * 4 > len(t):
        return None
    ip.update(sport=int.from_bytes(t[0:2], "big"), dport=int.from_bytes(t[2:4], "big"),
              seq=int.from_bytes(t[4:8], "big"), ack=int.from_bytes(t[8:12], "big"), b12=t[12], ctl=t[13],
              window=int.from_bytes(t[14:16], "big"), urgent=int.from_bytes(t[18:20], "big"),
              opts=bytes(t[20:doff * 4]), payload=bytes(t[doff * 4:]))
    ip["pay"] = len(ip["payload"])
    return ip


def same(a, b, ipver: int) -> bool:
    """same(i, i-1) for a = frame i and b = frame i-1 (parse results; None = not a member)."""
    if a is None or b is None:
        return False
    if a["src"] != b["src"] or a["dst"] != b["dst"] or a["ttl"] != b["ttl"]:
        return False
    if ipver == 4:
        if a["ihl"] != 20 or b["ihl"] != 20 or a["tos"] != b["tos"] or a["b67"] != b["b67"]:
            return False
        if a["ident"] != (b["ident"] + 1) % 65536:
            return False
    elif a["vcf"] != b["vcf"]:
        return False
    for k in ("sport", "dport", "ack", "window", "urgent", "b12", "opts"):
        if a[k] != b[k]:
            return False
    if a["seq"] != (b["seq"] + b["pay"]) % (1 << 32):
        return False
    if b["ctl"] & (FIN | SYN | RST | PSH | URG) or a["ctl"] & (SYN | RST | URG | CWR):
        return False
    return (a["ctl"] ^ b["ctl"]) & (0xFF ^ (FIN | PSH | CWR)) == 0


def gro(buf, offsets, valid, ipver: int) -> dict:
    """The outputs of the device call over frames buf[offsets[i], offsets[i+1]), exactly sized: per-super-segment
    arrays of n_super entries, offsets of n_super + 1, opts / data of their packed lengths, frame_seg of n."""
    buf = np.asarray(buf, np.uint8)
    offsets = np.asarray(offsets, np.uint64)
    n = offsets.size - 1
    ok = valid_bits(valid, n)
    fr = [parse(buf[int(offsets[i]):int(offsets[i + 1])].tobytes(), ipver) if ok[i] else None for i in range(n)]
    sm = [i >= 1 and same(fr[i], fr[i - 1], ipver) for i in range(n)]
    join = [False] * n
    for i in range(1, n):
        if not sm[i] or not 1 <= fr[i]["pay"] <= fr[i - 1]["pay"]:
            continue
        if i >= 2 and sm[i - 1] and fr[i - 1]["pay"] < fr[i - 2]["pay"]:
            continue  # frame i-1 was itself a short tail
        join[i] = True
    heads = [i for i in range(n) if fr[i] is not None and not join[i]]
    ns = len(heads)
    alen = 4 if ipver == 4 else 16
    out = {k: np.zeros(ns, dt) for k, dt in PER_SUPER}
    out["src"], out["dst"] = np.zeros((ns, alen), np.uint8), np.zeros((ns, alen), np.uint8)
    out["opt_off"], out["data_off"] = np.zeros(ns + 1, np.uint64), np.zeros(ns + 1, np.uint64)
    out["frame_seg"] = np.full(n, NONE, np.uint32)
    opts, data = [], []
    for s, f in enumerate(heads):
        l = f
        while l + 1 < n and join[l + 1]:
            l += 1
        a, z = fr[f], fr[l]
        out["src"][s], out["dst"][s] = np.frombuffer(a["src"], np.uint8), np.frombuffer(a["dst"], np.uint8)
        for k, v in (("ident", a["ident"]), ("ttl", a["ttl"]), ("tclass", a["tclass"]), ("flow", a["flow"]),
                     ("src_port", a["sport"]), ("dst_port", a["dport"]), ("seq_num", a["seq"]), ("ack_num", a["ack"]),
                     ("offset", a["b12"]), ("control", a["ctl"] | (z["ctl"] & (FIN | PSH))), ("window", a["window"]),
                     ("urgent_ptr", a["urgent"]), ("mss", max(a["pay"], 1)), ("first_frame", f),
                     ("frame_cnt", l - f + 1)):
            out[k][s] = v
        opts.append(a["opts"])
        data.extend(fr[i]["payload"] for i in range(f, l + 1))
        out["opt_off"][s + 1] = out["opt_off"][s] + np.uint64(len(a["opts"]))
        out["data_off"][s + 1] = out["data_off"][s] + np.uint64(sum(fr[i]["pay"] for i in range(f, l + 1)))
        out["frame_seg"][f:l + 1] = s
    out["opts"] = np.frombuffer(b"".join(opts), np.uint8).copy()
    out["data"] = np.frombuffer(b"".join(data), np.uint8).copy()
    out["n_super"] = ns
    return out


def as_batch(out: dict, ipver: int):
    """The outputs as the super-segment batch segmentation offload takes (a tests/_tso.Batch): the arrays straight
    through, frame_first the prefix sum of frame_cnt."""
    ns = int(out["n_super"])
    s = _tx.Case.__new__(_tx.Case)
    s.ipver, s.n = ipver, ns
    s.data = np.asarray(out["data"], np.uint8)
    s.data_off = np.asarray(out["data_off"], np.uint64)[:ns + 1]
    s.opts = np.concatenate([np.asarray(out["opts"], np.uint8), np.zeros(1, np.uint8)])  # never an empty array
    s.opt_off = np.asarray(out["opt_off"], np.uint64)[:ns + 1]
    s.fields = {k: np.asarray(out[k])[:ns] for k in ("src_port", "dst_port", "seq_num", "ack_num", "offset",
                                                       "control", "window", "urgent_ptr")}
    s.ip = {k: np.asarray(out[k])[:ns] for k in ("src", "dst", "ident", "ttl", "tclass", "flow")}
    b = _tso.Batch.__new__(_tso.Batch)
    b.sup, b.ipver, b.n = s, ipver, ns
    b.mss = np.asarray(out["mss"], np.uint32)[:ns]
    b.first = np.zeros(ns + 1, np.uint64)
    b.first[1:] = np.cumsum(np.asarray(out["frame_cnt"], np.uint64)[:ns])
    b.seg, b.off = _tso.layout(s.data_off, b.mss, b.first, s.opt_off, _tx.IPH[ipver])
    b.nf = int(b.first[-1])
    return b


def wire_offset(case):
    """Byte 12 of every segment of a tests/_tx.Case as TCP puts it on the wire: the header length in 32-bit words in
    the HIGH nibble (RFC 9293 §3.1). The reference's computeOffset() stores the count in the whole byte (tcp.go:59-66,
    :106), which a receiver reads as data offset 0: such a frame passes the receive pass and is no member here."""
    case.fields["offset"] = (case.fields["offset"].astype(np.uint8) << np.uint8(4)).astype(np.uint8)
    return case


def flow_case(rng, ipver: int, pays, opt: bytes = b"", ctl: int = ACK, seq0=None, ident0=None):
    """A tests/_tx.Case whose frames are one connection's segments in order: every field that of frame 0, sequence
    numbers continuing by the payload lengths, IPv4 idents counting up (both wrap)."""
    pays = [int(p) for p in pays]
    c = _tx.Case(rng, ipver, pays, opts=[opt] * len(pays))
    for d in (c.fields, c.ip):
        for v in d.values():
            v[:] = v[0]
    c.fields["control"][:] = ctl
    seq0 = int(c.fields["seq_num"][0]) if seq0 is None else seq0
    ident0 = int(c.ip["ident"][0]) if ident0 is None else ident0
    before = np.concatenate([[0], np.cumsum(pays)[:-1]]).astype(np.uint64)
    c.fields["seq_num"] = ((np.uint64(seq0) + before) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    c.ip["ident"] = ((ident0 + np.arange(len(pays))) & 0xFFFF).astype(np.uint16)
    return wire_offset(c)


def case_frames(c):
    """The list of frames (bytes) the transmit pass makes of a tests/_tx.Case."""
    off = c.packed()
    buf, _ = _tx.expected(c, off)
    return [buf[int(o):int(o) + int(L)].tobytes() for o, L in zip(off[:-1], c.flen)]


def pack(frames, lead: int = 0):
    """Frames packed back to back behind `lead` bytes (and three after): (buf, offsets)."""
    offs = np.zeros(len(frames) + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames]) if frames else []
    offs += np.uint64(lead)
    return np.frombuffer(b"\xEE" * lead + b"".join(frames) + b"\xEE" * 3, np.uint8).copy(), offs


def refix(f, ipver: int) -> bytes:
    """The frame with its IPv4 header checksum and its TCP checksum recomputed (whatever else was changed in it)."""
    from oracle import csum_oracle as O
    f = bytearray(f)
    if ipver == 4:
        ihl = (f[0] & 15) * 4
        f[10:12] = b"\0\0"
        f[10:12] = O.field_value(O.go_checksum(b"", bytes(f[:ihl]))).to_bytes(2, "big")
        ph = O.ipv4_pseudo_header(bytes(f[12:16]), bytes(f[16:20]), 6, len(f) - ihl)
    else:
        ihl = 40
        ph = O.ipv6_pseudo_header(bytes(f[8:24]), bytes(f[24:40]), 6, len(f) - 40)
    f[ihl + 16:ihl + 18] = b"\0\0"
    f[ihl + 16:ihl + 18] = O.field_value(O.go_checksum(ph, bytes(f[ihl:]))).to_bytes(2, "big")
    return bytes(f)


def dense(buf, off, flen):
    """Frames of flen[f] bytes at off[f] packed back to back: (bytes, offsets)."""
    parts = [np.asarray(buf[int(o):int(o) + int(L)]) for o, L in zip(off[:-1], flen)]
    offs = np.zeros(len(parts) + 1, np.uint64)
    offs[1:] = np.cumsum([p.size for p in parts])
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), offs


MSS_SET = (1460, 1448, 1461, 537, 3)
OPT_KEYS = ("mss", "nop_nop_k2len10", "k2len40")  # serialised lengths 4, 12 and 40: multiples of 4 that fit doff
CTLS = (0x10, 0x18, 0x11, 0x19, 0x90, 0x50, 0xD9, 0x00, 0x01, 0x08, 0x80)  # no SYN / RST / URG


def _cut_lengths(mss):
    """0, 1, mss − 1, mss, mss + 1, 3·mss and 3·mss ± 1 (the cut points of one super-segment)."""
    return sorted({0, 1, max(mss - 1, 0), mss, mss + 1, 3 * mss - 1, 3 * mss, 3 * mss + 1})


def cut_batch(ipver, mss, opts, lead=0, seed=0):
    """Every cut length of one mss, twice over in mixed order, control bytes from CTLS, option sets of 4-multiple
    length (and none)."""
    rng = np.random.default_rng(0x600 + 16 * mss + 2 * ipver + opts + 1000 * seed)
    lens = np.array(_cut_lengths(mss) * 2)
    rng.shuffle(lens)
    ob = None
    if opts:
        ob = [_tx.opt_bytes(rng, OPT_KEYS[i % len(OPT_KEYS)]) if i % 4 else b"" for i in range(lens.size)]
        assert all(len(x) % 4 == 0 for x in ob)
    b = _tso.Batch(rng, ipver, lens, mss, opts=ob, lead=lead)
    b.sup.fields["control"][:] = np.resize(np.array(CTLS, np.uint8), b.n)
    wire_offset(b.sup)
    return b


def cycle_connections(ipver, n, conns=4, cycle=(8, 8, 8, 8, 8, 8, 5), seed=0x7C0):
    """n frames as `conns` connections of near-equal size (one list of frames each), every connection's payloads
    cycling through `cycle`: with six 8s and a 5, every seventh frame is a short tail that ends a run."""
    rng = np.random.default_rng(seed + ipver)
    sizes = [n // conns + (i < n % conns) for i in range(conns)]
    return [case_frames(flow_case(rng, ipver, np.resize(np.array(cycle), k))) for k in sizes if k]


def frames_of(b, lead=0, rng=None):
    """The frames segmentation offload makes of batch b, packed densely behind `lead` bytes: (buf, offsets, valid
    bits)."""
    buf, _, c = _tso.expected(b)
    body, offs = dense(buf, b.off, c.flen)
    pad = np.full(lead, 0xEE, np.uint8) if rng is None else rng.integers(0, 256, lead, dtype=np.uint8)
    return np.concatenate([pad, body, np.full(3, 0xEE, np.uint8)]), offs + np.uint64(lead), np.ones(b.nf, bool)
