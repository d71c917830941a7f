"""Expected frames of the fused transmit pass (nsx_tx_ipv4_tcp_build_* / nsx_tx_ipv6_tcp_build_*), on the CPU.

The TCP images and raw sums come from the Go-faithful sender loop (O.c_go_tcp_build_mt: tcp.go:98-128 bytes(),
:72-95 computeChecksum, :110 the field) run over each frame's own pseudo-header, written IP-header-length bytes
into the frame's slot; the IP headers are written here in numpy (RFC 791 §3.1 / RFC 8200 §3). The self-checks of
tests/test_tx_abi.py hold this module to O.ipv4_tcp_frame / O.ipv6_tcp_frame byte for byte and to the receive
oracle (O.c_rx_ipv4_tcp / O.c_rx_ipv6_tcp: every expected frame valid)."""
import numpy as np

from oracle import csum_oracle as O

IPH = {4: 20, 6: 40}
WIRE_MAX = {4: 65515, 6: 65535}  # the longest TCP part the IP length field can carry

OPT_SETS = {  # tests/test_gpu_parity.py _OPT_SETS restated: option lists as the reference serialises them
    "nop_nop_k2len10": lambda r: [O.Option(kind=1), O.Option(kind=1), O.Option(kind=2, length=10, data=r(8))],
    "mss": lambda r: [O.Option(kind=2, length=4, data=r(2))],
    "nop_nop": lambda r: [O.Option(kind=1)] * 2,           # 22 B header: 2 pad bytes, still 4-aligned
    "nop": lambda r: [O.Option(kind=1)],                   # 21 B + 1 pad: a 22 B header (general path)
    "nop3": lambda r: [O.Option(kind=1)] * 3,              # 23 B + 3 pad: 26 B
    "k2len40": lambda r: [O.Option(kind=2, length=40, data=r(38))],  # 60 B header, the TCP maximum
    "k2len41": lambda r: [O.Option(kind=2, length=41, data=r(39))],  # 61 B + 1 pad: 62 B header
    "k2len100": lambda r: [O.Option(kind=2, length=100, data=r(98))],  # 120 B header, 4-aligned
}


def opt_bytes(rng, key):
    rb = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    return b"".join(o.bytes() for o in OPT_SETS[key](rb))


def wire_len(olen, dlen):
    """nsx_tcp_wire_len restated (tcp.go:98-128: 20 + options + `remainder` padding + payload)."""
    olen, dlen = np.asarray(olen, np.uint64), np.asarray(dlen, np.uint64)
    return 20 + olen + np.where(olen > 0, (20 + olen) % 4, 0).astype(np.uint64) + dlen


class Case:
    """One batch: TCP fields, options, payloads and IP fields as host arrays."""

    def __init__(self, rng, ipver, lens, opts=None, lead=0):
        """lens: payload bytes per frame; opts: per-frame option serialisations (bytes; b"" = none) or None for a
        batch without an option array; lead: bytes before the first payload (the payload source alignment)."""
        n = len(lens)
        self.ipver, self.n = ipver, n
        lens = np.asarray(lens, np.uint64)
        self.data = rng.integers(0, 256, lead + int(lens.sum()) + 8, dtype=np.uint8)
        self.data_off = np.zeros(n + 1, np.uint64)
        self.data_off[1:] = np.cumsum(lens)
        self.data_off += np.uint64(lead)
        self.fields = {k: rng.integers(0, 1 << (8 * np.dtype(dt).itemsize), n, dtype=np.uint64).astype(dt)
                       for k, dt in zip(O.TCP_FIELDS, O.TCP_FIELD_DTYPES)}
        self.opts = self.opt_off = None
        olen = np.zeros(n, np.uint64)
        if opts is not None:
            olen = np.array([len(b) for b in opts], np.uint64)
            self.opts = np.frombuffer(b"\x77" + b"".join(opts) + b"\x77", np.uint8).copy()  # at odd addresses
            self.opt_off = np.zeros(n + 1, np.uint64)
            self.opt_off[1:] = np.cumsum(olen)
            self.opt_off += np.uint64(1)
        self.fields["offset"] = ((20 + olen + 3) // 4).astype(np.uint8)  # computeOffset (tcp.go:59-66)
        self.wire = wire_len(olen, lens)
        self.flen = self.wire + np.uint64(IPH[ipver])
        alen = 4 if ipver == 4 else 16
        self.ip = {"src": rng.integers(0, 256, (n, alen), dtype=np.uint8),
                   "dst": rng.integers(0, 256, (n, alen), dtype=np.uint8),
                   "ident": rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16),
                   "ttl": rng.integers(0, 256, n, dtype=np.uint8),
                   "tclass": rng.integers(0, 256, n, dtype=np.uint8),
                   "flow": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)}  # bits above 20 ignored

    def packed(self):
        """nsx_tx_layout_host restated: out_off[i] = Σ_{j<i} round_up4(ip_hdr_len + wire_j)."""
        off = np.zeros(self.n + 1, np.uint64)
        off[1:] = np.cumsum((self.flen + np.uint64(3)) & ~np.uint64(3))
        return off


def be16(v):
    v = np.asarray(v, np.uint64)
    return np.stack([(v >> np.uint64(8)) & np.uint64(0xFF), v & np.uint64(0xFF)], 1).astype(np.uint8)


def pseudo_headers(case):
    """(n, 12) RFC 9293 §3.1 or (n, 40) RFC 8200 §8.1 pseudo-headers from the frames' own addresses, protocol 6 and
    TCP length."""
    n, w = case.n, case.wire
    if case.ipver == 4:
        return np.ascontiguousarray(np.concatenate(
            [case.ip["src"], case.ip["dst"], np.zeros((n, 1), np.uint8), np.full((n, 1), 6, np.uint8), be16(w)], 1))
    return np.ascontiguousarray(np.concatenate(
        [case.ip["src"], case.ip["dst"], be16(w >> np.uint64(16)), be16(w), np.zeros((n, 3), np.uint8),
         np.full((n, 1), 6, np.uint8)], 1))


def hdr_checksum(h):
    """go_checksum (tcp.go:72-95) over each row of an (n, even) byte matrix, vectorised: BE words, end-around carry."""
    w = h.astype(np.uint64)
    s = ((w[:, 0::2] << np.uint64(8)) | w[:, 1::2]).sum(1)
    for _ in range(3):
        s = (s & np.uint64(0xFFFF)) + (s >> np.uint64(16))
    return s.astype(np.uint16)


def ip_headers(case, ident=None, ttl=None, tclass=None, flow=None):
    """(n, 20) IPv4 or (n, 40) IPv6 header bytes; the optional fields default to the case's arrays."""
    n = case.n
    ttl = case.ip["ttl"] if ttl is None else np.broadcast_to(np.asarray(ttl, np.uint8), n)
    if case.ipver == 4:
        ident = case.ip["ident"] if ident is None else np.broadcast_to(np.asarray(ident, np.uint16), n)
        h = np.zeros((n, 20), np.uint8)
        h[:, 0] = 0x45
        h[:, 2:4] = be16(case.wire + np.uint64(20))
        h[:, 4:6] = be16(ident)
        h[:, 6] = 0x40  # DF, fragment offset 0
        h[:, 8] = ttl
        h[:, 9] = 6     # ip.NextProtoTCP (protocols.go:8)
        h[:, 12:16] = case.ip["src"]
        h[:, 16:20] = case.ip["dst"]
        h[:, 10:12] = be16(~hdr_checksum(h))  # RFC 791 §3.1: ~sum over the header with the field zero
        return h
    tclass = case.ip["tclass"] if tclass is None else np.broadcast_to(np.asarray(tclass, np.uint8), n)
    flow = case.ip["flow"] if flow is None else np.broadcast_to(np.asarray(flow, np.uint32), n)
    vtf = (np.uint64(6) << np.uint64(28)) | (tclass.astype(np.uint64) << np.uint64(20)) | \
        (flow.astype(np.uint64) & np.uint64(0xFFFFF))
    h = np.zeros((n, 40), np.uint8)
    h[:, 0:2] = be16(vtf >> np.uint64(16))
    h[:, 2:4] = be16(vtf)
    h[:, 4:6] = be16(case.wire)
    h[:, 6] = 6
    h[:, 7] = ttl
    h[:, 8:24] = case.ip["src"]
    h[:, 24:40] = case.ip["dst"]
    return h


def expected(case, off, fill=0, **ip_overrides):
    """The output buffer and TCP raw sums the transmit pass must produce for frames at off[i] (4-aligned slots)
    over a buffer pre-filled with `fill`: each built frame, then zeros up to the next multiple of 4, everything
    else untouched; a frame whose TCP part exceeds the IP length field is not built (slot untouched, raw 0).
    Returns (buf[off[n]], raw[n])."""
    iph = IPH[case.ipver]
    off = np.asarray(off, np.uint64)
    z, raw = O.c_go_tcp_build_mt(case.fields, case.data, case.data_off, off + np.uint64(iph), pseudo_headers(case),
                                 opts=case.opts, opt_off=case.opt_off)
    hdr = ip_headers(case, **ip_overrides)
    built = case.wire <= np.uint64(WIRE_MAX[case.ipver])
    out = np.full(int(off[-1]), fill, np.uint8)
    for i in np.nonzero(built)[0]:
        o, L = int(off[i]), int(case.flen[i])
        pad = (L + 3) & ~3
        out[o:o + iph] = hdr[i]
        out[o + iph:o + L] = z[o + iph:o + L]
        out[o + L:o + pad] = 0
    raw = raw.copy()
    raw[~built] = 0
    return out, raw
