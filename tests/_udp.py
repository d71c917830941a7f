"""The UDP passes (nsx_udp_tx_* / nsx_udp_uso_* / nsx_udp_rx_*) restated on the CPU, in numpy, from the contract
comment of include/nsx_csum.h alone: the expected output buffer and raw sums of the transmit pass and of segmentation
offload, and the expected mask and raw sums of the receive verify.

The IP headers are tests/_tx.ip_headers' (the header the TCP transmit pass writes) with the protocol byte 17 and the
length of the UDP datagram, the IPv4 header checksum redone with tests/_tx.hdr_checksum; every other sum is `raw`
below, the serial computeChecksum loop (tcp.go:72-95: big-endian words, odd tail zero-padded, end-around carry). A
super-datagram batch is expanded on the CPU into the per-frame batch and then built frame by frame, as tests/_tso.py
does. tests/test_udp_abi.py holds this module to nsx.csum16 and to the oracle's IPv4 header checksum, and its receive
side to its transmit side. No torch and no GPU at import."""
import types

import numpy as np

import _tso
import _tx

IPH = _tx.IPH
PAY_MAX = {4: 65507, 6: 65527}  # the longest payload the IP length field can carry
NO_CSUM = 1


def raw(b):
    """computeChecksum over the bytes b (the pseudo-header already in front): 0 only for all-zero input."""
    b = np.asarray(b, np.uint8)
    if b.size & 1:
        b = np.append(b, np.uint8(0))
    w = b.astype(np.uint64)
    s = int(((w[0::2] << np.uint64(8)) | w[1::2]).sum())
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


class Case:
    """One per-frame batch: ports, IP fields and payloads as host arrays. Frame i's payload is data[lo[i], hi[i]);
    data_off (n + 1) is the one offsets array the device call takes (lo = data_off[:-1], hi = data_off[1:]) — an
    expanded super-datagram batch whose frame map lies has none."""

    def __init__(self, rng, ipver, lens, lead=0):
        n = len(lens)
        self.ipver, self.n = ipver, n
        lens = np.asarray(lens, np.uint64)
        self.data = rng.integers(0, 256, lead + int(lens.sum()) + 8, dtype=np.uint8)
        self.data_off = np.zeros(n + 1, np.uint64)
        self.data_off[1:] = np.cumsum(lens)
        self.data_off += np.uint64(lead)
        self.lo, self.hi = self.data_off[:-1].copy(), self.data_off[1:].copy()
        self.ports = {k: rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16)
                      for k in ("src_port", "dst_port")}
        alen = 4 if ipver == 4 else 16
        self.ip = {"src": rng.integers(0, 256, (n, alen), dtype=np.uint8),
                   "dst": rng.integers(0, 256, (n, alen), dtype=np.uint8),
                   "ident": rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16),
                   "ttl": rng.integers(0, 256, n, dtype=np.uint8),
                   "tclass": rng.integers(0, 256, n, dtype=np.uint8),
                   "flow": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)}

    @property
    def plen(self):
        return (self.hi - self.lo).astype(np.uint64)

    @property
    def flen(self):
        return self.plen + np.uint64(IPH[self.ipver] + 8)

    def packed(self):
        """nsx_udp_layout_host restated: out_off[i] = Σ_{j<i} round_up4(ip_hdr_len + 8 + len_j)."""
        return layout(self.data_off, IPH[self.ipver])


def layout(data_off, ip_hdr_len):
    lens = np.diff(np.asarray(data_off, np.uint64)).astype(np.uint64)
    off = np.zeros(lens.size + 1, np.uint64)
    off[1:] = np.cumsum((lens + np.uint64(ip_hdr_len + 8 + 3)) & ~np.uint64(3))
    return off


def ip_headers(c, null=()):
    """(n, 20) / (n, 40): the TCP transmit pass's header with the protocol / Next Header 17 and the UDP datagram's
    length. null: the optional nsx_ip_hdr_soa members passed as NULL (ident 0, ttl 64, tclass 0, flow 0)."""
    shim = types.SimpleNamespace(ipver=c.ipver, n=c.n, ip=c.ip, wire=(c.plen + np.uint64(8)) & np.uint64(0xFFFF))
    over = {k: v for k, v in (("ident", 0), ("ttl", 64), ("tclass", 0), ("flow", 0)) if k in null}
    h = _tx.ip_headers(shim, **over)
    if c.ipver == 4:
        h[:, 9] = 17
        h[:, 10:12] = 0
        h[:, 10:12] = _tx.be16(~_tx.hdr_checksum(h))  # RFC 791 §3.1
    else:
        h[:, 6] = 17
    return h


def pseudo(ipver, src, dst, ulen):
    """The pseudo-header bytes of one frame: src dst 0 17 len(2), or RFC 8200 §8.1's src dst len(4) 0 0 0 17."""
    src, dst = np.asarray(src, np.uint8), np.asarray(dst, np.uint8)
    if ipver == 4:
        return np.concatenate([src, dst, np.array([0, 17, ulen >> 8, ulen & 0xFF], np.uint8)])
    return np.concatenate([src, dst, np.array([0, 0, ulen >> 8, ulen & 0xFF, 0, 0, 0, 17], np.uint8)])


def datagram(c, i, field=0):
    """Frame i's UDP datagram with the given checksum field."""
    p = c.data[int(c.lo[i]):int(c.hi[i])]
    ulen = 8 + p.size
    sp, dp = int(c.ports["src_port"][i]), int(c.ports["dst_port"][i])
    h = np.array([sp >> 8, sp & 0xFF, dp >> 8, dp & 0xFF, ulen >> 8, ulen & 0xFF, field >> 8, field & 0xFF], np.uint8)
    return np.concatenate([h, p])


def frame_raw(c, i):
    """raw of frame i: over the pseudo-header ‖ the datagram with the field zero."""
    d = datagram(c, i)
    return raw(np.concatenate([pseudo(c.ipver, c.ip["src"][i], c.ip["dst"][i], d.size), d]))


def frames(c, flags=0, null=()):
    """Per frame the built bytes (None for a frame that is not built) and the raw sums."""
    hdr = ip_headers(c, null)
    out, raws = [], np.zeros(c.n, np.uint16)
    for i in range(c.n):
        if int(c.plen[i]) > PAY_MAX[c.ipver]:
            out.append(None)
            continue
        r = frame_raw(c, i)
        assert r != 0  # the pseudo-header holds the byte 17
        field = ~r & 0xFFFF
        field = field or 0xFFFF  # RFC 768
        if flags & NO_CSUM:
            assert c.ipver == 4
            field = 0
        raws[i] = r
        out.append(np.concatenate([hdr[i], datagram(c, i, field)]))
    return out, raws


def expected(c, off, fill=0, flags=0, null=(), total=None):
    """The output buffer (off[n] bytes, or `total`) and raw sums the transmit pass must produce over a buffer
    pre-filled with `fill`: each built frame, zeros up to the next multiple of 4, everything else untouched."""
    off = np.asarray(off, np.uint64)
    fr, raws = frames(c, flags, null)
    out = np.full(int(off[-1]) if total is None else total, fill, np.uint8)
    for i, f in enumerate(fr):
        if f is None:
            continue
        o = int(off[i])
        out[o:o + f.size] = f
        out[o + f.size:o + ((f.size + 3) & ~3)] = 0
    return out, raws


def craft_ffff(c, i, pos):
    """Set the two payload bytes at payload offset pos of frame i so that raw == 0xFFFF: the computed checksum is
    0 and the stored field must be 0xFFFF. pos even: one aligned word; odd: the low byte of one word and the high
    byte of the next. Asserts that the craft worked."""
    a = int(c.lo[i]) + pos
    assert pos + 2 <= int(c.plen[i])
    c.data[a:a + 2] = 0
    v = 0xFFFF - frame_raw(c, i)
    c.data[a:a + 2] = (v >> 8, v & 0xFF) if pos % 2 == 0 else (v & 0xFF, v >> 8)
    assert frame_raw(c, i) == 0xFFFF


# ------------------------------------------------------------------ segmentation offload
class Batch:
    """n super-datagrams: a Case whose every entry is one super-datagram (`sup`) and gso[s]."""

    def __init__(self, rng, ipver, lens, gso, lead=0):
        self.sup = Case(rng, ipver, lens, lead=lead)
        self.ipver, self.n = ipver, self.sup.n
        self.gso = np.broadcast_to(np.asarray(gso, np.uint32), self.n).copy()
        self.first = _tso.count(self.sup.data_off, self.gso)  # nsx_tso_count_host's map, as it stands
        self.seg, self.off = uso_layout(self.sup.data_off, self.gso, self.first, IPH[ipver])
        self.nf = int(self.first[-1])


def uso_layout(data_off, gso, first, ip_hdr_len):
    """nsx_udp_uso_layout_host restated: (frame_seg u32, out_off u64)."""
    seg, _ = _tso.frame_index(first)
    lo, hi = _tso.slices(data_off, gso, first)
    off = np.zeros(seg.size + 1, np.uint64)
    off[1:] = np.cumsum(((hi - lo).astype(np.uint64) + np.uint64(ip_hdr_len + 8 + 3)) & ~np.uint64(3))
    return seg.astype(np.uint32), off


def expand(b, null=(), seg=None):
    """The per-frame Case of batch b. seg: the frame map's frame_seg as the device sees it (default: the true one);
    frame f is built from super-datagram seg[f] with j = f - first[seg[f]] modulo 2^64, its slice clamped to the
    super-datagram's own range."""
    s = b.sup
    seg = np.asarray(b.seg if seg is None else seg, np.int64)
    c = Case.__new__(Case)
    c.ipver, c.n, c.data = b.ipver, seg.size, s.data
    lo, hi, ident = [], [], []
    for f, q in enumerate(seg.tolist()):
        j = (f - int(b.first[q])) % (1 << 64)
        d0, d1, g = int(s.data_off[q]), int(s.data_off[q + 1]), int(b.gso[q])
        a = min(d0 + j * g, d1)
        lo.append(a)
        hi.append(min(a + g, d1))
        ident.append(((0 if "ident" in null else int(s.ip["ident"][q])) + j) & 0xFFFF)
    c.lo, c.hi = np.array(lo, np.uint64), np.array(hi, np.uint64)
    c.data_off = None
    if seg.size and np.array_equal(c.lo[1:], c.hi[:-1]):
        c.data_off = np.concatenate([c.lo, c.hi[-1:]]).astype(np.uint64)
    c.ports = {k: np.ascontiguousarray(v[seg]) for k, v in s.ports.items()}
    c.ip = {k: np.ascontiguousarray(v[seg]) for k, v in s.ip.items()}
    c.ip["ident"] = np.array(ident, np.uint16)
    return c


def uso_expected(b, off=None, fill=0, flags=0, null=(), seg=None, total=None):
    """(buf, raw, case): `expected` over the expanded batch. `ident` in null is applied by the expansion."""
    c = expand(b, null, seg)
    buf, raws = expected(c, b.off if off is None else off, fill=fill, flags=flags,
                         null=tuple(k for k in null if k != "ident"), total=total)
    return buf, raws, c


# ------------------------------------------------------------------ receive verify
def rx_expected(ipver, buf, offs):
    """(valid bool[n], ip_raw u16[n], udp_raw u16[n]) of the receive verify over frames buf[offs[i], offs[i+1])."""
    buf = np.asarray(buf, np.uint8)
    n = len(offs) - 1
    valid, ipr, udr = np.zeros(n, bool), np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    for i in range(n):
        p = buf[int(offs[i]):int(offs[i + 1])]
        L = p.size
        if ipver == 4:
            if L < 20:
                continue
            ihl = (int(p[0]) & 15) * 4
            if ihl < 20 or ihl > L:
                continue
            ipr[i] = raw(p[:ihl])
            wf = (p[0] >> 4) == 4 and ((int(p[2]) << 8) | int(p[3])) == L and \
                (((int(p[6]) << 8) | int(p[7])) & 0x3FFF) == 0 and p[9] == 17
            src, dst, hl = p[12:16], p[16:20], ihl
        else:
            wf = L >= 48 and (p[0] >> 4) == 6 and 40 + ((int(p[4]) << 8) | int(p[5])) == L and p[6] == 17
            if not wf:
                continue
            src, dst, hl = p[8:24], p[24:40], 40
        P = L - hl
        if not wf or P < 8:
            continue
        U = (int(p[hl + 4]) << 8) | int(p[hl + 5])
        if not 8 <= U <= P:
            continue
        field = (int(p[hl + 6]) << 8) | int(p[hl + 7])
        r = raw(np.concatenate([pseudo(ipver, src, dst, U), p[hl:hl + U]]))  # bytes past U are padding
        udr[i] = r
        if ipver == 4:
            valid[i] = ipr[i] == 0xFFFF and (r == 0xFFFF or field == 0)
        else:
            valid[i] = r == 0xFFFF and field != 0
    return valid, ipr, udr


def concat(frs, lead=0, rng=None):
    """Frames (byte arrays) packed densely behind `lead` junk bytes: (buf, offs)."""
    lens = [len(f) for f in frs]
    offs = np.zeros(len(frs) + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    offs += np.uint64(lead)
    junk = rng.integers(0, 256, lead, dtype=np.uint8) if rng is not None else np.zeros(lead, np.uint8)
    buf = np.concatenate([junk] + [np.asarray(f, np.uint8) for f in frs]) if frs else junk
    return buf.astype(np.uint8), offs


# ------------------------------------------------------------------ receive: edge frames and corruptions
def fix4(f):
    """The IPv4 frame f with its header checksum redone over the IHL*4 bytes it claims (where it holds them)."""
    f = np.array(f, np.uint8)
    ihl = (int(f[0]) & 15) * 4 if f.size else 0
    if 20 <= ihl <= f.size:
        f[10:12] = 0
        r = raw(f[:ihl])
        f[10:12] = ((~r >> 8) & 0xFF, ~r & 0xFF)
    return f


def set_len(f, ipver, L):
    """The frame with its IP length field saying L bytes of frame (IPv4 header checksum redone)."""
    f = np.array(f, np.uint8)
    if ipver == 4:
        f[2:4] = (L >> 8, L & 0xFF)
        return fix4(f)
    f[4:6] = ((L - 40) >> 8, (L - 40) & 0xFF)
    return f


CORRUPTIONS = ("none", "payload_byte", "ip_header_bit", "field_zero", "field_zero_bad_payload", "udp_len_short",
               "udp_len_long", "udp_len_trim", "protocol", "length_field", "truncate", "version", "padding")


def corrupt(rng, f, ipver, kind):
    """Frame f (as the transmit pass built it) with one corruption of CORRUPTIONS; IP-level fields other than the
    one corrupted stay consistent, so that the verdict hangs on that one thing."""
    f = np.array(f, np.uint8)
    h = IPH[ipver]
    P = f.size - h
    if kind == "none":
        return f
    if kind == "payload_byte":  # one bit of the ports or the payload (P >= 8): the sum moves by a power of two
        k = int(rng.integers(P - 4))
        f[h + (k if k < 4 else k + 4)] ^= np.uint8(1 << int(rng.integers(8)))
    elif kind == "ip_header_bit":  # no fix: IPv4's header checksum catches it; IPv6 only where the bit matters
        f[int(rng.integers(h))] ^= np.uint8(1 << int(rng.integers(8)))
    elif kind == "field_zero":
        f[h + 6:h + 8] = 0
    elif kind == "field_zero_bad_payload":
        f[h + 6:h + 8] = 0
        f[h + (8 + int(rng.integers(P - 8)) if P > 8 else 0)] ^= np.uint8(0x10)
    elif kind == "udp_len_short":
        U = int(rng.integers(8))
        f[h + 4:h + 6] = (0, U)
    elif kind == "udp_len_long":
        U = P + 1 + int(rng.integers(4))
        f[h + 4:h + 6] = ((U >> 8) & 0xFF, U & 0xFF)
    elif kind == "udp_len_trim":  # a shorter U that is still >= 8: the checksum no longer matches (almost surely)
        U = 8 + int(rng.integers(max(P - 8, 1)))
        f[h + 4:h + 6] = (U >> 8, U & 0xFF)
    elif kind == "protocol":
        f[9 if ipver == 4 else 6] = 6
        f = fix4(f) if ipver == 4 else f
    elif kind == "length_field":
        f = set_len(f, ipver, f.size + (1 if f.size < 65535 else -1))
    elif kind == "truncate":
        f = f[:int(rng.integers(f.size))]
    elif kind == "version":
        f[0] = (f[0] & 0x0F) | (0x60 if ipver == 4 else 0x40)
        f = fix4(f) if ipver == 4 else f
    elif kind == "padding":  # junk behind the datagram, the IP length saying so: still valid
        f = np.concatenate([f, rng.integers(0, 256, 1 + int(rng.integers(9)), dtype=np.uint8)])
        f = set_len(f, ipver, f.size)
    else:
        raise ValueError(kind)
    return f


def rx_edge_frames(ipver, seed=0):
    """[(name, frame)] — the receive pass's edge cases for one IP version, each built from valid frames of `frames`."""
    rng = np.random.default_rng([0x0ED6E, ipver, seed])
    h = IPH[ipver]
    lens = [0, 1, 7, 100, 1472, 33, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, PAY_MAX[ipver], 247, 248, 249]
    c = Case(rng, ipver, lens, lead=1)
    craft_ffff(c, 6, 10)
    fr, _ = frames(c)
    out = [("valid_%d" % lens[i], fr[i]) for i in (0, 1, 2, 3, 4, 5, 20, 21, 22)]  # 248: a datagram of 256 bytes
    out.append(("field_ffff_crafted", fr[6]))
    assert fr[6][h + 6] == 0xFF and fr[6][h + 7] == 0xFF
    g = fr[7].copy(); g[h + 8 + 5] ^= 0x40
    out.append(("wrong_payload_byte", g))
    if ipver == 4:
        g = fr[8].copy(); g[10] ^= 0x01
        out.append(("wrong_header_checksum", g))
    out.append(("field_zero", corrupt(rng, fr[9], ipver, "field_zero")))
    out.append(("field_zero_any_raw", corrupt(rng, fr[9], ipver, "field_zero_bad_payload")))
    out.append(("u_eq_p", fr[10]))
    out.append(("u_lt_p_junk_padding", corrupt(rng, fr[10], ipver, "padding")))
    g = fr[11].copy(); g[h + 4:h + 6] = (0, 7)
    out.append(("u_lt_8", g))
    g = fr[11].copy(); g[h + 4:h + 6] = (0, 73)
    out.append(("u_gt_p", g))
    out.append(("protocol_6", corrupt(rng, fr[12], ipver, "protocol")))
    out.append(("length_mismatch", corrupt(rng, fr[13], ipver, "length_field")))
    out.append(("wrong_version", corrupt(rng, fr[14], ipver, "version")))
    if ipver == 4:
        g = fr[15].copy(); g[6] |= 0x20
        out.append(("fragment_mf", fix4(g)))
        g = fr[15].copy(); g[7] = 3
        out.append(("fragment_offset", fix4(g)))
        g = fr[15].copy(); g[6] = 0x1F  # the high bits of the offset, DF cleared
        out.append(("fragment_offset_high", fix4(g)))
        g = np.concatenate([fr[16][:20], np.array([1, 1, 1, 0], np.uint8), fr[16][20:]])
        g[0] = 0x46
        out.append(("ihl6_options", set_len(g, 4, g.size)))
        g = fr[17].copy(); g[0] = 0x44
        out.append(("ihl_lt_5", g))
        out += [("len_0", fr[0][:0]), ("len_27", fr[0][:27]), ("len_28", fr[0])]
    else:
        out += [("len_0", fr[0][:0]), ("len_47", fr[0][:47]), ("len_48", fr[0])]
    out.append(("frame_64k", fr[19]))
    return out
