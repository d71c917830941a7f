"""Seeded batches for the ICMP fuzz (tests/test_gpu_icmp_fuzz.py) and for the edge-case GPU tests: frames of every
kind the three passes tell apart, built with tests/_icmp.py. tests/test_icmp_gen.py shows on any host that no seed is
vacuous. No torch and no GPU at import."""
import numpy as np

import _icmp as M

SEEDS = 20
RX_KINDS = {4: ("valid", "bad_icmp_sum", "bad_ip_sum", "truncated", "too_short", "wrong_proto", "fragment", "mf",
                "bad_version", "bad_len", "bad_ihl", "garbage"),
            6: ("valid", "bad_icmp_sum", "truncated", "too_short", "wrong_proto", "bad_version", "bad_len", "garbage")}
ERR_KINDS = ("udp", "icmp_query", "icmp_error", "icmp_no_type", "fragment", "first_fragment", "src_zero", "src_mcast",
             "dst_mcast", "short", "bad_version", "bad_len", "garbage")


def tune(rng):
    """Random launch overrides of nsx_icmp_tune.h (None = the product call)."""
    if rng.random() < 0.25:
        return None
    return dict(blocks_per_cu=int(rng.choice([0, 1, 2, 8])), run_segs=int(rng.choice([0, 1, 7, 16, 17, 64, 300])))


def _addr(rng, ipver, first=None):
    a = bytearray(rng.integers(0, 256, 4 if ipver == 4 else 16, dtype=np.uint8).tobytes())
    a[0] = int(rng.integers(1, 224)) if first is None else first
    return bytes(a)


def _pay(rng, hi):
    return rng.integers(0, 256, int(rng.integers(0, hi + 1)), dtype=np.uint8).tobytes()


def _opts(rng):
    return rng.integers(0, 256, 4 * int(rng.choice([0, 0, 0, 1, 10])), dtype=np.uint8).tobytes()


def icmp_frame(rng, ipver, type_, code=0, data=b"", src=None, dst=None, **kw):
    """A valid IPv4 / IPv6 frame carrying one ICMP message with random rest-of-header bytes."""
    src = _addr(rng, ipver) if src is None else src
    dst = _addr(rng, ipver) if dst is None else dst
    rest = rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
    if ipver == 4:
        return M.ip4(1, src, dst, M.icmp4(type_, code, rest, data), ttl=int(rng.integers(0, 256)),
                     ident=int(rng.integers(1 << 16)), flags_off=int(rng.choice([0, 0x4000, 0x8000])), **kw)
    return M.ip6(58, src, dst, M.icmp6(type_, code, rest, data, src, dst), hop=int(rng.integers(0, 256)),
                 flow=int(rng.integers(1 << 20)), tclass=int(rng.integers(256)))


def rx_frame(rng, kind, ipver, max_pay=300):
    """One frame of a verify kind: "valid" verifies, every other kind fails in exactly the way its name says."""
    types = (0, 3, 8, 11, 12, 13) if ipver == 4 else (1, 2, 3, 4, 128, 129, 135)
    kw = dict(options=_opts(rng)) if ipver == 4 else {}
    f = bytearray(icmp_frame(rng, ipver, int(rng.choice(types)), int(rng.integers(0, 6)), _pay(rng, max_pay), **kw))
    ihl = (f[0] & 15) * 4 if ipver == 4 else 40
    if kind == "valid":
        return bytes(f)
    if kind == "bad_icmp_sum":
        f[int(rng.integers(ihl, len(f)))] ^= int(rng.integers(1, 256))
    elif kind == "bad_ip_sum":
        f[int(rng.choice([1, 4, 5, 8, 10, 11, 12, 19]))] ^= int(rng.integers(1, 256))
    elif kind == "truncated":  # the frame ends before the length field says
        f = f[:len(f) - int(rng.integers(1, 9))]
    elif kind == "too_short":  # fewer than 8 ICMP bytes, the lengths consistent
        g = M.ip4(1, bytes(f[12:16]), bytes(f[16:20]), bytes(f[ihl:ihl + int(rng.integers(0, 8))])) if ipver == 4 else \
            M.ip6(58, bytes(f[8:24]), bytes(f[24:40]), bytes(f[40:40 + int(rng.integers(0, 8))]))
        return g
    elif kind == "wrong_proto":
        at = 9 if ipver == 4 else 6
        f[at] = int(rng.choice([6, 17, 2, 58 if ipver == 4 else 1]))
        if ipver == 4:
            f[10:12] = b"\0\0"
            f[10:12] = M.field(M.raw(f[:ihl])).to_bytes(2, "big")
    elif kind in ("fragment", "mf"):
        w = int.from_bytes(f[6:8], "big") | (int(rng.integers(1, 0x2000)) if kind == "fragment" else 0x2000)
        f[6:8] = w.to_bytes(2, "big")
        f[10:12] = b"\0\0"
        f[10:12] = M.field(M.raw(f[:ihl])).to_bytes(2, "big")
    elif kind == "bad_version":
        f[0] = (f[0] & 15) | (int(rng.choice([0, 5, 6 if ipver == 4 else 4, 15])) << 4)
    elif kind == "bad_len":
        at = 2 if ipver == 4 else 4
        v = int.from_bytes(f[at:at + 2], "big")
        f[at:at + 2] = ((v + int(rng.choice([-1, 1, 4, 256]))) & 0xFFFF).to_bytes(2, "big")
    elif kind == "bad_ihl":
        f[0] = 0x40 | int(rng.choice([0, 1, 4, 15]))
        if (f[0] & 15) * 4 + 8 <= len(f) and (f[0] & 15) >= 5:  # IHL 15 over a frame that holds it: not this kind
            f[0] = 0x44
    elif kind == "garbage":
        return rng.integers(0, 256, int(rng.integers(0, 80)), dtype=np.uint8).tobytes()
    else:
        raise ValueError(kind)
    return bytes(f)


def rx_batch(seed, ipver, n=None):
    """(buf, offs, kinds): about 600 frames, every kind of RX_KINDS at least twice, behind 0-3 lead bytes."""
    rng = np.random.default_rng([0x1C3F, 1, ipver, seed])
    n = int(rng.integers(500, 700)) if n is None else n
    kinds = list(RX_KINDS[ipver]) * 2 + list(rng.choice(RX_KINDS[ipver], n - 2 * len(RX_KINDS[ipver]),
                                                        p=_weights(len(RX_KINDS[ipver]))))
    kinds = [kinds[i] for i in rng.permutation(n)]
    fr = [rx_frame(rng, k, ipver, max_pay=int(rng.choice([40, 300, 300, 3000]))) for k in kinds]
    buf, offs = M.pack(fr, lead=int(rng.integers(4)), tail=int(rng.integers(4)))
    return buf, offs, kinds


def _weights(k):
    w = np.ones(k)
    w[0] = k  # half of the frames are valid
    return w / w.sum()


def err_frame(rng, kind, ipver, max_pay=700):
    """One offending frame of an error-generation kind (tests/_icmp.py pre_status says what becomes of it)."""
    mc = 0xFF if ipver == 6 else int(rng.integers(224, 256))
    pay = _pay(rng, max_pay)
    if kind in ("udp", "fragment", "first_fragment", "src_zero", "src_mcast", "dst_mcast"):
        src = _addr(rng, ipver, mc) if kind == "src_mcast" else bytes(4 if ipver == 4 else 16) if kind == "src_zero" \
            else _addr(rng, ipver)
        dst = _addr(rng, ipver, mc) if kind == "dst_mcast" else _addr(rng, ipver)
        if ipver == 6:
            return M.ip6(int(rng.choice([6, 17, 44])), src, dst, pay, hop=int(rng.integers(256)))
        w = {"fragment": int(rng.integers(1, 0x2000)) | int(rng.choice([0, 0x2000])), "first_fragment": 0x2000}.get(kind, 0)
        return M.ip4(int(rng.choice([6, 17])), src, dst, pay, ttl=int(rng.integers(256)), flags_off=w, options=_opts(rng))
    if kind == "icmp_query":
        return icmp_frame(rng, ipver, int(rng.choice(M.QUERY4 if ipver == 4 else (128, 129, 133, 136))), 0, pay)
    if kind == "icmp_error":
        return icmp_frame(rng, ipver, int(rng.choice((3, 4, 5, 11, 12, 40, 255) if ipver == 4 else (1, 2, 3, 4, 127, 137))),
                          0, pay)
    if kind == "icmp_no_type":
        return M.ip4(1, _addr(rng, 4), _addr(rng, 4), b"", options=_opts(rng)) if ipver == 4 else \
            M.ip6(58, _addr(rng, 6), _addr(rng, 6), b"")
    f = bytearray(err_frame(rng, "udp", ipver, max_pay))
    if kind == "short":
        return bytes(f[:int(rng.integers(0, 20 if ipver == 4 else 40))])
    if kind == "bad_version":
        f[0] = (f[0] & 15) | (int(rng.choice([0, 5, 6 if ipver == 4 else 4])) << 4)
    elif kind == "bad_len":
        return bytes(f) + b"\0" if rng.random() < 0.5 else bytes(f[:-1]) if len(f) > (20 if ipver == 4 else 40) else \
            bytes(f) + b"\0\0"
    elif kind == "garbage":
        return rng.integers(0, 256, int(rng.integers(0, 100)), dtype=np.uint8).tobytes()
    return bytes(f)


def requests(rng, n, ipver, p_none=0.25, p_bad=0.1):
    """Request and argument words: allowed types with random codes, zeros, and refused words (unknown types, high
    bits)."""
    types = M.ALLOWED[ipver]
    req = np.array([int(rng.choice(types)) | int(rng.integers(0, 256)) << 8 for _ in range(n)], np.uint32)
    u = rng.random(n)
    req[u < p_none] = 0
    bad = (u >= p_none) & (u < p_none + p_bad)
    for i in np.nonzero(bad)[0]:
        req[i] = int(rng.choice([5, 8, 0x80, 0xFF, 11 | 1 << 16, 3 | 1 << 31, 1 << 24]))
    arg = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return req, arg


def err_batch(seed, ipver, n=None):
    """(buf, offs, req, arg, kw): about 500 frames of every kind of ERR_KINDS, requests of every sort, and a cap below
    the eligible count, so that all five statuses occur."""
    rng = np.random.default_rng([0x1C3F, 2, ipver, seed])
    n = int(rng.integers(400, 600)) if n is None else n
    kinds = list(ERR_KINDS) * 2 + list(rng.choice(ERR_KINDS, n - 2 * len(ERR_KINDS), p=_weights(len(ERR_KINDS))))
    kinds = [kinds[i] for i in rng.permutation(n)]
    fr = [err_frame(rng, k, ipver, max_pay=int(rng.choice([60, 700, 700, 1600]))) for k in kinds]
    req, arg = requests(rng, n, ipver)
    buf, offs = M.pack(fr, lead=int(rng.integers(4)), tail=int(rng.integers(4)))
    eligible = sum(M.pre_status(f, int(r), ipver) == M.SENT for f, r in zip(fr, req))
    kw = dict(src=_addr(rng, ipver), ttl=int(rng.integers(256)), ident0=int(rng.integers(1 << 32)),
              max_out=int(rng.integers(eligible // 2, eligible - 4)))  # five or more are LIMITED
    return buf, offs, req, (None if rng.random() < 0.2 else arg), kw


def echo_batch(seed, ipver, n=None):
    """(buf, offs, valid, ttl): about 600 frames — echo requests of every payload length (IPv4: with options too),
    some to a multicast address, some with a wrong checksum, replies and other ICMP, and the malformed kinds of the
    verify — and a valid mask that is mostly the truth, with bits set over frames that do not verify and clear over
    some that do."""
    rng = np.random.default_rng([0x1C3F, 3, ipver, seed])
    n = int(rng.integers(500, 700)) if n is None else n
    rq, mc = (8, bytes([224, 0, 0, 251])) if ipver == 4 else (128, bytes([0xFF, 2] + [0] * 13 + [1]))
    fr = []
    for i in range(n):
        u = rng.random()
        kw = dict(options=_opts(rng)) if ipver == 4 else {}
        if u < 0.5:
            f = icmp_frame(rng, ipver, rq, 0, _pay(rng, 200), **kw)
        elif u < 0.58:
            f = icmp_frame(rng, ipver, rq, 0, _pay(rng, 60), dst=mc, **kw)
        elif u < 0.66:
            f = icmp_frame(rng, ipver, rq, int(rng.integers(1, 256)), _pay(rng, 60), **kw)
        elif u < 0.75:
            g = bytearray(icmp_frame(rng, ipver, rq, 0, _pay(rng, 60), **kw))
            ihl = (g[0] & 15) * 4 if ipver == 4 else 40
            at = int(rng.choice([ihl + 2, ihl + 3, len(g) - 1] + ([10, 11] if ipver == 4 else [])))
            g[at] ^= int(rng.integers(1, 256))
            f = bytes(g)
        else:
            f = rx_frame(rng, str(rng.choice(RX_KINDS[ipver])), ipver, 100)
        fr.append(f)
    buf, offs = M.pack(fr, lead=int(rng.integers(4)), tail=int(rng.integers(4)))
    valid = M.verify(buf, offs, ipver)["ok"]
    flip = rng.random(n) < 0.15
    return buf, offs, valid ^ flip, int(rng.integers(256))
