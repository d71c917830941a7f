"""UDP receive coalescing (nsx_ugro_ipv4_dev / nsx_ugro_ipv6_dev and the flow-keyed nsx_ugro_flow_*) restated in numpy and
plain Python from the contract comment of include/nsx_csum.h alone: member, same(i, i-1), join(i) with its three-frame
window, every output array, the flow key and the stable order — frame by frame, without looking at the library.
tests/test_ugro_abi.py holds it to UDP segmentation offload's expansion (tests/_udp.py): coalescing the frames of a
super-datagram batch gives the batch back. No torch and no GPU at import."""
import numpy as np

import _gro
import _gro_flow
import _tso
import _udp

NONE = 0xFFFFFFFF
NO_FLOW = 0xFFFFFFFF
IPH = _udp.IPH
PER_SUPER = (("ident", np.uint16), ("ttl", np.uint8), ("tclass", np.uint8), ("flow", np.uint32),
             ("src_port", np.uint16), ("dst_port", np.uint16), ("gso", np.uint32), ("first_frame", np.uint64),
             ("frame_cnt", np.uint32))
valid_bits = _gro.valid_bits


def parse(f: bytes, ipver: int):
    """The member's view of one frame whose valid bit is set, or None: well-formed as the UDP receive verify defines,
    U == P and a checksum field that is not 0."""
    f = bytes(f)
    L = len(f)
    if ipver == 4:
        if L < 20 or f[0] >> 4 != 4:
            return None
        ihl = (f[0] & 15) * 4
        if ihl < 20 or ihl > L or int.from_bytes(f[2:4], "big") != L:
            return None
        if f[6] & 0x20 or (f[6] & 0x1F) or f[7] or f[9] != 17 or L - ihl < 8:
            return None
        ip = dict(src=f[12:16], dst=f[16:20], ttl=f[8], ihl=ihl, tos=f[1], b67=f[6:8],
                  ident=int.from_bytes(f[4:6], "big"), tclass=f[1], flow=0)
    else:
        if L < 48 or f[0] >> 4 != 6 or 40 + int.from_bytes(f[4:6], "big") != L or f[6] != 17:
            return None
        ihl = 40
        w = int.from_bytes(f[0:4], "big")
        ip = dict(src=f[8:24], dst=f[24:40], ttl=f[7], vcf=f[0:4], ident=0, tclass=(w >> 20) & 0xFF, flow=w & 0xFFFFF)
    u = f[ihl:]
    P, U = len(u), int.from_bytes(u[4:6], "big")
    if not 8 <= U <= P or U != P or u[6:8] == b"\0\0":
        return None
    ip.update(sport=int.from_bytes(u[0:2], "big"), dport=int.from_bytes(u[2:4], "big"), payload=u[8:], pay=U - 8)
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
    return a["sport"] == b["sport"] and a["dport"] == b["dport"]


def ugro(buf, offsets, valid, ipver: int) -> dict:
    """The outputs of the adjacent device call over frames buf[offsets[i], offsets[i+1]), exactly sized: per-super-
    datagram arrays of n_super entries, data_off of n_super + 1, data of its packed length, frame_seg of n."""
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
    out["data_off"] = np.zeros(ns + 1, np.uint64)
    out["frame_seg"] = np.full(n, NONE, np.uint32)
    data = []
    for s, f in enumerate(heads):
        l = f
        while l + 1 < n and join[l + 1]:
            l += 1
        a = fr[f]
        out["src"][s], out["dst"][s] = np.frombuffer(a["src"], np.uint8), np.frombuffer(a["dst"], np.uint8)
        for k, v in (("ident", a["ident"]), ("ttl", a["ttl"]), ("tclass", a["tclass"]), ("flow", a["flow"]),
                     ("src_port", a["sport"]), ("dst_port", a["dport"]), ("gso", max(a["pay"], 1)),
                     ("first_frame", f), ("frame_cnt", l - f + 1)):
            out[k][s] = v
        data.extend(fr[i]["payload"] for i in range(f, l + 1))
        out["data_off"][s + 1] = out["data_off"][s] + np.uint64(sum(fr[i]["pay"] for i in range(f, l + 1)))
        out["frame_seg"][f:l + 1] = s
    out["data"] = np.frombuffer(b"".join(data), np.uint8).copy()
    out["n_super"] = ns
    return out


# ------------------------------------------------------------------ the flow-keyed form
def key(frame: bytes, ipver: int) -> int:
    """The flow key of a frame whose valid bit is set: tests/_gro_flow's arithmetic (FNV-1a over the little-endian
    address dwords, then the dword at the transport header's start — here the two UDP ports); 0xFFFFFFFF unless it is
    a member."""
    if parse(frame, ipver) is None:
        return NO_FLOW
    return _gro_flow._mix(_gro_flow.state(frame, ipver), _gro_flow._dwords(frame, ipver)[-1])


def keys(buf, offsets, valid, ipver: int):
    buf = np.asarray(buf, np.uint8)
    offsets = np.asarray(offsets, np.uint64)
    n = offsets.size - 1
    ok = valid_bits(valid, n)
    return np.array([key(buf[int(offsets[i]):int(offsets[i + 1])].tobytes(), ipver) if ok[i] else NO_FLOW
                     for i in range(n)], np.uint32).reshape(n)


def order(buf, offsets, valid, ipver: int):
    """The stable ascending sort of the frame indices by key (uint32)."""
    return np.argsort(keys(buf, offsets, valid, ipver), kind="stable").astype(np.uint32)


def ugro_flow(buf, offsets, valid, ipver: int) -> dict:
    """The outputs of the flow-keyed device call: `ugro` over the frames repacked in key order (first_frame holds
    positions in that order), frame_seg turned back to the original frame indices, plus `order`."""
    buf = np.asarray(buf, np.uint8)
    offsets = np.asarray(offsets, np.uint64)
    n = offsets.size - 1
    ok = valid_bits(valid, n)
    od = order(buf, offsets, valid, ipver)
    frames = [buf[int(offsets[f]):int(offsets[f + 1])].tobytes() for f in od]
    buf2, offs2 = _gro.pack(frames)
    out = ugro(buf2, offs2, ok[od], ipver)
    seg = np.full(n, NONE, np.uint32)
    seg[od] = out["frame_seg"]
    out["frame_seg"] = seg
    out["order"] = od
    return out


def as_batch(out: dict, ipver: int):
    """The outputs as the super-datagram batch UDP segmentation offload takes (a tests/_udp.Batch): the arrays
    straight through, frame_first the prefix sum of frame_cnt — which must be the map nsx_tso_count_host makes of
    data_off and gso."""
    ns = int(out["n_super"])
    s = _udp.Case.__new__(_udp.Case)
    s.ipver, s.n = ipver, ns
    s.data = np.asarray(out["data"], np.uint8)
    s.data_off = np.asarray(out["data_off"], np.uint64)[:ns + 1].copy()
    s.lo, s.hi = s.data_off[:-1].copy(), s.data_off[1:].copy()
    s.ports = {k: np.asarray(out[k], np.uint16)[:ns] for k in ("src_port", "dst_port")}
    alen = 4 if ipver == 4 else 16
    s.ip = {k: np.asarray(out[k])[:ns] for k in ("ident", "ttl", "tclass", "flow")}
    s.ip["src"] = np.asarray(out["src"], np.uint8).reshape(-1)[:ns * alen].reshape(ns, alen)
    s.ip["dst"] = np.asarray(out["dst"], np.uint8).reshape(-1)[:ns * alen].reshape(ns, alen)
    b = _udp.Batch.__new__(_udp.Batch)
    b.sup, b.ipver, b.n = s, ipver, ns
    b.gso = np.asarray(out["gso"], np.uint32)[:ns].copy()
    b.first = np.zeros(ns + 1, np.uint64)
    b.first[1:] = np.cumsum(np.asarray(out["frame_cnt"], np.uint64)[:ns])
    assert np.array_equal(b.first, _tso.count(s.data_off, b.gso)), "frame_cnt is not segmentation offload's count"
    b.seg, b.off = _udp.uso_layout(s.data_off, b.gso, b.first, IPH[ipver])
    b.nf = int(b.first[-1])
    return b


# ------------------------------------------------------------------ frames to test with
def flow_case(rng, ipver: int, pays, ident0=None, lead=0):
    """A tests/_udp.Case whose frames are one flow's datagrams in order: every field that of frame 0, IPv4 idents
    counting up (they wrap). IPv4 TOS is what the transmit pass writes, 0."""
    c = _udp.Case(rng, ipver, [int(p) for p in pays], lead=lead)
    for d in (c.ports, c.ip):
        for v in d.values():
            v[:] = v[0]
    ident0 = int(c.ip["ident"][0]) if ident0 is None else ident0
    c.ip["ident"] = ((ident0 + np.arange(c.n)) & 0xFFFF).astype(np.uint16)
    return c


def case_frames(c, flags=0):
    """The list of frames (bytes) the UDP transmit pass makes of a tests/_udp.Case."""
    fr, _ = _udp.frames(c, flags)
    return [f.tobytes() for f in fr]


def flow_frames(rng, ipver: int, pays, ident0=None):
    return case_frames(flow_case(rng, ipver, pays, ident0))


def pack(frames, lead: int = 0, exact: bool = False):
    """Frames packed back to back behind `lead` bytes (and three after, unless exact): (buf, offsets)."""
    buf, offs = _gro.pack(frames, lead=lead)
    return (buf[:buf.size - 3].copy() if exact else buf), offs


def refix(f, ipver: int) -> bytes:
    """The frame with its IPv4 header checksum and its UDP checksum recomputed over the UDP length it states (whatever
    else was changed in it); a computed 0 is stored as 0xFFFF."""
    f = np.frombuffer(bytes(f), np.uint8).copy()
    if ipver == 4:
        f = _udp.fix4(f)
        ihl, src, dst = (int(f[0]) & 15) * 4, f[12:16], f[16:20]
    else:
        ihl, src, dst = 40, f[8:24], f[24:40]
    U = (int(f[ihl + 4]) << 8) | int(f[ihl + 5])
    f[ihl + 6:ihl + 8] = 0
    r = _udp.raw(np.concatenate([_udp.pseudo(ipver, src, dst, U), f[ihl:ihl + U]]))
    v = (~r & 0xFFFF) or 0xFFFF
    f[ihl + 6:ihl + 8] = (v >> 8, v & 0xFF)
    return f.tobytes()


def with_ports(frame: bytes, ipver: int, ports: int) -> bytes:
    """The frame with its UDP bytes 0-3 replaced by the dword `ports` (little-endian), checksums re-fixed."""
    f = bytearray(frame)
    ihl = (f[0] & 15) * 4 if ipver == 4 else 40
    f[ihl:ihl + 4] = int(ports).to_bytes(4, "little")
    return refix(f, ipver)


def frames_of(b, lead=0):
    """The frames UDP segmentation offload makes of batch b, packed densely behind `lead` bytes: (buf, offsets)."""
    buf, _, c = _udp.uso_expected(b)
    body, offs = _gro.dense(buf, b.off, c.flen)
    return np.concatenate([np.full(lead, 0xEE, np.uint8), body, np.full(3, 0xEE, np.uint8)]), offs + np.uint64(lead)
