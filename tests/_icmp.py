"""The ICMP family (include/nsx_csum.h nsx_icmp_*) restated in numpy / plain Python, independent of the kernels: error
generation, the request helpers, the receive verify and the in-place echo reply, written from the header comment and
the RFCs it names (792, 1122 §3.2.2, 1191, 1812 §4.3.2, 4443 §2.4, 8200 §8.1, 1624). Every sum is the oracle's raw sum
(oracle/csum_oracle.py fold_checksum), used read-only. tests/test_icmp_abi.py holds this file to known answers and to
the models that exist already (tests/_frag.py, tests/_nat.py); the GPU tests compare the kernels against it.

No torch and no GPU at import."""
import numpy as np

from oracle import csum_oracle as O

NONE, SENT, QUIET, BAD, LIMITED = 0, 1, 2, 3, 4
HDR = {4: 28, 6: 48}
QUOTE = {4: 548, 6: 1232}
ALLOWED = {4: (3, 11, 12), 6: (1, 2, 3, 4)}
QUERY4 = (0, 8, 9, 10, 13, 14, 15, 16, 17, 18)  # the ICMP types an error may be sent about (RFC 1122 §3.2.2)
FILL = 0xA5
FRAG_DF = 2


def raw(b: bytes, prefix: bytes = b"") -> int:
    """The raw sum over prefix ‖ b, an odd tail padded with a zero byte."""
    return O.fold_checksum(prefix, bytes(b))


def field(r: int) -> int:
    return ~r & 0xFFFF


def pseudo6(src: bytes, dst: bytes, length: int) -> bytes:
    """RFC 8200 §8.1: src, dst, the 32-bit upper-layer length, three zero bytes, next header 58."""
    return bytes(src) + bytes(dst) + length.to_bytes(4, "big") + b"\0\0\0\x3a"


# ---------------------------------------------------------------- frames
def ip4(proto: int, src: bytes, dst: bytes, payload: bytes, ttl: int = 64, ident: int = 0, flags_off: int = 0x4000,
        options: bytes = b"", tos: int = 0) -> bytes:
    """An IPv4 datagram with a valid header checksum; flags_off is the word at bytes 6-7 (default: DF)."""
    assert len(options) % 4 == 0 and len(options) <= 40
    ihl = 5 + len(options) // 4
    h = bytearray(bytes([0x40 | ihl, tos]) + (4 * ihl + len(payload)).to_bytes(2, "big") + ident.to_bytes(2, "big") +
                  flags_off.to_bytes(2, "big") + bytes([ttl, proto, 0, 0]) + bytes(src) + bytes(dst) + options)
    h[10:12] = field(raw(h)).to_bytes(2, "big")
    return bytes(h) + bytes(payload)


def ip6(nh: int, src: bytes, dst: bytes, payload: bytes, hop: int = 64, flow: int = 0, tclass: int = 0) -> bytes:
    vtf = (6 << 28) | (tclass << 20) | flow
    return vtf.to_bytes(4, "big") + len(payload).to_bytes(2, "big") + bytes([nh, hop]) + bytes(src) + bytes(dst) + \
        bytes(payload)


def icmp4(type_: int, code: int, rest: bytes, data: bytes = b"") -> bytes:
    """An ICMP message with a valid checksum: type, code, checksum, the 4 `rest` bytes, data."""
    assert len(rest) == 4
    m = bytearray(bytes([type_, code, 0, 0]) + bytes(rest) + bytes(data))
    m[2:4] = field(raw(m)).to_bytes(2, "big")
    return bytes(m)


def icmp6(type_: int, code: int, rest: bytes, data: bytes, src: bytes, dst: bytes) -> bytes:
    assert len(rest) == 4
    m = bytearray(bytes([type_, code, 0, 0]) + bytes(rest) + bytes(data))
    m[2:4] = field(raw(m, pseudo6(src, dst, len(m)))).to_bytes(2, "big")
    return bytes(m)


def echo4(src: bytes, dst: bytes, ident: int = 1, seq: int = 1, data: bytes = b"", ttl: int = 64, reply: bool = False,
          options: bytes = b"", ip_ident: int = 0) -> bytes:
    rest = ident.to_bytes(2, "big") + seq.to_bytes(2, "big")
    return ip4(1, src, dst, icmp4(0 if reply else 8, 0, rest, data), ttl=ttl, options=options, ident=ip_ident)


def echo6(src: bytes, dst: bytes, ident: int = 1, seq: int = 1, data: bytes = b"", hop: int = 64,
          reply: bool = False, flow: int = 0) -> bytes:
    rest = ident.to_bytes(2, "big") + seq.to_bytes(2, "big")
    return ip6(58, src, dst, icmp6(129 if reply else 128, 0, rest, data, src, dst), hop=hop, flow=flow)


def pack(fr, lead: int = 0, tail: int = 3, fill: int = FILL):
    """Frames packed back to back behind `lead` fill bytes, `tail` fill bytes after: (buf, offsets)."""
    offs = np.zeros(len(fr) + 1, np.uint64)
    if fr:
        offs[1:] = np.cumsum([len(f) for f in fr])
    offs += np.uint64(lead)
    buf = np.frombuffer(bytes([fill]) * lead + b"".join(bytes(f) for f in fr) + bytes([fill]) * tail, np.uint8).copy()
    return buf, offs


def frames_of(buf, offs):
    buf = np.asarray(buf, np.uint8)
    return [buf[int(offs[i]):int(offs[i + 1])].tobytes() if int(offs[i + 1]) > int(offs[i]) else b""
            for i in range(len(offs) - 1)]


# ---------------------------------------------------------------- error generation
def malformed(f: bytes, ipver: int) -> bool:
    L = len(f)
    if ipver == 4:
        return L < 20 or f[0] >> 4 != 4 or (f[0] & 15) < 5 or (f[0] & 15) * 4 > L or int.from_bytes(f[2:4], "big") != L
    return L < 40 or f[0] >> 4 != 6 or 40 + int.from_bytes(f[4:6], "big") != L


def quiet(f: bytes, ipver: int, type_: int, code: int) -> bool:
    """The RFCs' silence rules over a frame that is not malformed."""
    if ipver == 4:
        ihl = (f[0] & 15) * 4
        if int.from_bytes(f[6:8], "big") & 0x1FFF:  # RFC 1122 §3.2.2: a non-initial fragment
            return True
        if f[12:16] == b"\0\0\0\0" or f[12] >= 224:  # RFC 1812 §4.3.2.7: a source that names no single host
            return True
        if f[16] >= 224:  # RFC 1122 §3.2.2: a datagram destined to a multicast (or class E / broadcast) address
            return True
        if f[9] == 1 and (ihl >= len(f) or f[ihl] not in QUERY4):  # RFC 1122 §3.2.2: an ICMP error message
            return True
        return False
    if f[8:24] == bytes(16) or f[8] == 0xFF:  # RFC 4443 §2.4(e.6)
        return True
    if f[24] == 0xFF and not (type_ == 2 or (type_ == 4 and code == 2)):  # RFC 4443 §2.4(e.3)
        return True
    if f[6] == 58 and (len(f) <= 40 or f[40] < 128 or f[40] == 137):  # RFC 4443 §2.4(e.1), (e.2)
        return True
    return False


def pre_status(f: bytes, r: int, ipver: int) -> int:
    """NONE, BAD, QUIET, or SENT for a frame that is eligible (the cap not yet applied)."""
    if r == 0:
        return NONE
    type_, code = r & 0xFF, (r >> 8) & 0xFF
    if r >> 16 or type_ not in ALLOWED[ipver] or malformed(f, ipver):
        return BAD
    return QUIET if quiet(f, ipver, type_, code) else SENT


def message(f: bytes, r: int, a: int, src: bytes, ttl: int, ident: int, ipver: int) -> bytes:
    """The message about frame f for request r with argument a."""
    q = f[:QUOTE[ipver]]
    body = bytes([r & 0xFF, (r >> 8) & 0xFF, 0, 0]) + (a & 0xFFFFFFFF).to_bytes(4, "big") + q
    if ipver == 4:
        m = bytearray(body)
        m[2:4] = field(raw(m)).to_bytes(2, "big")
        h = bytearray(b"\x45\xc0" + (28 + len(q)).to_bytes(2, "big") + (ident & 0xFFFF).to_bytes(2, "big") + b"\0\0" +
                      bytes([ttl, 1, 0, 0]) + bytes(src[:4]) + f[12:16])
        h[10:12] = field(raw(h)).to_bytes(2, "big")
        return bytes(h) + bytes(m)
    m = bytearray(body)
    m[2:4] = field(raw(m, pseudo6(src, f[8:24], len(m)))).to_bytes(2, "big")
    return b"\x60\0\0\0" + len(m).to_bytes(2, "big") + bytes([58, ttl]) + bytes(src) + f[8:24] + bytes(m)


def err(buf, offs, req, arg, src: bytes, ttl: int, ident0: int, max_out: int, ipver: int) -> dict:
    """The outputs of the device call, exactly sized: status (n), src_frame (n_out), out_off (n_out + 1), out (its
    packed bytes), n_out, and `msgs`, the messages as a list of bytes."""
    fr = frames_of(buf, offs)
    n = len(fr)
    arg = np.zeros(n, np.uint32) if arg is None else np.asarray(arg, np.uint32)
    status = np.zeros(n, np.uint8)
    src_frame, msgs = [], []
    rank = 0
    for i, f in enumerate(fr):
        r = int(req[i])
        st = pre_status(f, r, ipver)
        if st == SENT:
            if rank >= max_out:
                st = LIMITED
            else:
                msgs.append(message(f, r, int(arg[i]), src, ttl, ident0 + len(msgs), ipver))
                src_frame.append(i)
            rank += 1
        status[i] = st
    out_off = np.zeros(len(msgs) + 1, np.uint64)
    if msgs:
        out_off[1:] = np.cumsum([len(m) for m in msgs])
    return dict(status=status, src_frame=np.array(src_frame, np.uint32), out_off=out_off, n_out=len(msgs), msgs=msgs,
                out=np.frombuffer(b"".join(msgs), np.uint8))


def out_bytes_worst(fr, max_out: int, ipver: int) -> int:
    """The header comment's worst-case extent: every frame's message, whatever its status."""
    return sum(HDR[ipver] + min(len(f), QUOTE[ipver]) for f in fr)


# ---------------------------------------------------------------- request helpers
def req_frag(status, mtu, req, arg):
    req, arg = np.array(req, np.uint32), np.array(arg, np.uint32)
    hit = np.asarray(status) == FRAG_DF
    req[hit] = 3 | (4 << 8)
    arg[hit] = np.asarray(mtu, np.uint32)[hit] & np.uint32(0xFFFF)
    return req, arg


def whole_header(f: bytes, ipver: int) -> bool:
    if ipver == 4:
        return len(f) >= 20 and f[0] >> 4 == 4 and (f[0] & 15) >= 5 and (f[0] & 15) * 4 <= len(f)
    return len(f) >= 40 and f[0] >> 4 == 6


def req_ttl(buf, offs, valid, ttl_dec: int, req, arg, ipver: int):
    req, arg = np.array(req, np.uint32), np.array(arg, np.uint32)
    for i, f in enumerate(frames_of(buf, offs)):
        if valid[i] and whole_header(f, ipver) and (f[8] if ipver == 4 else f[7]) <= ttl_dec:
            req[i], arg[i] = (11 if ipver == 4 else 3), 0
    return req, arg


# ---------------------------------------------------------------- receive verify
def wellformed(f: bytes, ipver: int):
    """The IP header length of a frame that is well-formed as the verify defines (the sums are not looked at), else
    None."""
    L = len(f)
    if ipver == 4:
        if L < 20 or f[0] >> 4 != 4:
            return None
        ihl = (f[0] & 15) * 4
        if ihl < 20 or ihl + 8 > L or int.from_bytes(f[2:4], "big") != L:
            return None
        if int.from_bytes(f[6:8], "big") & 0x3FFF or f[9] != 1:
            return None
        return ihl
    if L < 48 or f[0] >> 4 != 6 or 40 + int.from_bytes(f[4:6], "big") != L or f[6] != 58:
        return None
    return 40


def verify_frame(f: bytes, ipver: int):
    """(ok, ip_raw, icmp_raw, type word) of one frame."""
    ip_raw = 0
    if ipver == 4 and len(f) >= 20 and 5 <= (f[0] & 15) and (f[0] & 15) * 4 <= len(f):
        ip_raw = raw(f[:(f[0] & 15) * 4])
    ihl = wellformed(f, ipver)
    if ihl is None:
        return False, ip_raw, 0, 0xFFFF
    r = raw(f[ihl:]) if ipver == 4 else raw(f[40:], pseudo6(f[8:24], f[24:40], len(f) - 40))
    ok = r == 0xFFFF and (ipver == 6 or ip_raw == 0xFFFF)
    return ok, ip_raw, r, ((f[ihl] << 8) | f[ihl + 1]) if ok else 0xFFFF


def verify(buf, offs, ipver: int) -> dict:
    res = [verify_frame(f, ipver) for f in frames_of(buf, offs)]
    return dict(ok=np.array([r[0] for r in res], bool), ip_raw=np.array([r[1] for r in res], np.uint16),
                icmp_raw=np.array([r[2] for r in res], np.uint16), type=np.array([r[3] for r in res], np.uint16))


# ---------------------------------------------------------------- echo reply
def fold(x: int) -> int:
    return 0 if x == 0 else 1 + (x - 1) % 0xFFFF


def update(hc: int, old: int, new: int) -> int:
    """RFC 1624 eqn. 3 over one 16-bit word old -> new."""
    return ~fold((~hc & 0xFFFF) + (~old & 0xFFFF) + new) & 0xFFFF


def echo_frame(f: bytes, ttl: int, ipver: int):
    """The reply written over request f (its valid bit set), or None when f is not answered."""
    ihl = wellformed(f, ipver)
    if ihl is None or f[ihl] != (8 if ipver == 4 else 128) or f[ihl + 1] != 0:
        return None
    g = bytearray(f)
    be = lambda b, k: int.from_bytes(b[k:k + 2], "big")  # noqa: E731
    if ipver == 4:
        if f[16] >= 224:
            return None
        g[12:16], g[16:20] = f[16:20], f[12:16]
        g[8] = ttl
        g[10:12] = update(be(f, 10), be(f, 8), be(g, 8)).to_bytes(2, "big")
        g[ihl] = 0
    else:
        if f[24] == 0xFF:
            return None
        g[8:24], g[24:40] = f[24:40], f[8:24]
        g[7] = ttl
        g[ihl] = 129
    g[ihl + 2:ihl + 4] = update(be(f, ihl + 2), be(f, ihl), be(g, ihl)).to_bytes(2, "big")
    return bytes(g)


def echo(buf, offs, valid, ttl: int, ipver: int):
    """(new_buf, hit): the whole buffer after the device call and n booleans, frame i answered."""
    out = np.asarray(buf, np.uint8).copy()
    fr = frames_of(buf, offs)
    hit = np.zeros(len(fr), bool)
    for i, f in enumerate(fr):
        g = echo_frame(f, ttl, ipver) if valid[i] else None
        if g is not None:
            out[int(offs[i]):int(offs[i + 1])] = np.frombuffer(g, np.uint8)
            hit[i] = True
    return out, hit


def rebuilt_reply(f: bytes, ttl: int, ipver: int) -> bytes:
    """The reply to request f built from scratch: every checksum recomputed over the new bytes."""
    if ipver == 4:
        ihl = (f[0] & 15) * 4
        return ip4(1, f[16:20], f[12:16], icmp4(0, 0, f[ihl + 4:ihl + 8], f[ihl + 8:]), ttl=ttl,
                   ident=int.from_bytes(f[4:6], "big"), flags_off=int.from_bytes(f[6:8], "big"),
                   options=f[20:ihl], tos=f[1])
    vtf = int.from_bytes(f[:4], "big")
    return ip6(58, f[24:40], f[8:24], icmp6(129, 0, f[44:48], f[48:], f[24:40], f[8:24]), hop=ttl,
               flow=vtf & 0xFFFFF, tclass=(vtf >> 20) & 0xFF)
