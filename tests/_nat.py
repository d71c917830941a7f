"""The in-place NAT rewrite (nsx_nat_table_build_host, nsx_nat_ipv4_tcp_rewrite_dev / nsx_nat_ipv6_tcp_rewrite_dev)
restated in numpy and plain Python from the comment in include/nsx_csum.h alone, without looking at the library: the
tuple, the table layout, the hash (tests/_gro_flow.py's flow key over the same dwords), the probe, the translated
condition and RFC 1624 eqn. 3 word by word. tests/test_nat_abi.py holds it to what exists: frames of the transmit
pass's model (tests/_tx.py), rewritten here, are the frames that model builds from the new fields."""
import numpy as np

import _gro
import _gro_flow as FL

TUPLE = {4: 12, 6: 36}
ENTRY = {4: 32, 6: 80}
FILL = 0xA5


def wellformed(f: bytes, ipver: int):
    """The IP header length of a frame that is well-formed as the receive pass of its IP version defines (length,
    version, protocol and fragment conditions; the checksums and the TCP data offset are not looked at), else None."""
    L = len(f)
    if ipver == 4:
        if L < 20 or f[0] >> 4 != 4:
            return None
        ihl = (f[0] & 15) * 4
        if ihl < 20 or ihl > L or int.from_bytes(f[2:4], "big") != L:
            return None
        if f[6] & 0x3F or f[7] or f[9] != 6 or L - ihl < 20:  # MF, fragment offset, protocol, segment length
            return None
        return ihl
    if L < 40 or f[0] >> 4 != 6 or 40 + int.from_bytes(f[4:6], "big") != L or f[6] != 6 or L - 40 < 20:
        return None
    return 40


def tuple_of(f: bytes, ipver: int, ihl=None) -> bytes:
    """src, dst and the two ports as they stand on the wire (a well-formed frame)."""
    ihl = ((f[0] & 15) * 4 if ipver == 4 else 40) if ihl is None else ihl
    return bytes(f[12:20] if ipver == 4 else f[8:40]) + bytes(f[ihl:ihl + 4])


def key(t: bytes) -> int:
    """FNV-1a over the tuple's little-endian dwords: nsx_gro_flow_*'s flow key."""
    h = FL.FNV_BASIS
    for k in range(0, len(t), 4):
        h = FL._mix(h, int.from_bytes(t[k:k + 4], "little"))
    return h


def _entry(table, slot: int, ipver: int):
    """(occupied, match tuple, new tuple) of one entry."""
    tb, eb = TUPLE[ipver], ENTRY[ipver]
    e = bytes(table[slot * eb:(slot + 1) * eb])
    return int.from_bytes(e[tb:tb + 4], "little") == 1, e[:tb], e[tb + 4:2 * tb + 4]


def build_table(ipver: int, match, new, slots: int) -> np.ndarray:
    """nsx_nat_table_build_host: zero-filled, the rules inserted in order, each into the first entry on its probe
    path that is not occupied. ValueError where the call returns NSX_EINVAL."""
    tb, eb = TUPLE[ipver], ENTRY[ipver]
    match, new = [bytes(m) for m in match], [bytes(m) for m in new]
    n = len(match)
    if slots < 16 or slots & (slots - 1) or slots < 2 * n or slots > 1 << 31:
        raise ValueError("slots")
    if len(set(match)) != n:
        raise ValueError("duplicate match tuple")
    table = np.zeros(slots * eb, np.uint8)
    for m, r in zip(match, new):
        assert len(m) == tb and len(r) == tb
        s = key(m) & (slots - 1)
        while _entry(table, s, ipver)[0]:
            s = (s + 1) & (slots - 1)
        table[s * eb:(s + 1) * eb] = np.frombuffer(m + (1).to_bytes(4, "little") + r + bytes(4), np.uint8)
    return table


def lookup(table, slots: int, t: bytes, ipver: int):
    """The new tuple for tuple t, or None: probe from the home slot; an entry that is not occupied is a miss, an
    occupied one with an equal match tuple a hit; after `slots` probes a miss — whatever bytes the table holds."""
    home = key(t) & (slots - 1)
    for p in range(slots):
        occ, m, r = _entry(table, (home + p) & (slots - 1), ipver)
        if not occ:
            return None
        if m == t:
            return r
    return None


def _words(b: bytes):
    return [int.from_bytes(b[k:k + 2], "big") for k in range(0, len(b), 2)]


def fold(x: int) -> int:
    return 0 if x == 0 else 1 + (x - 1) % 0xFFFF


def update(hc: int, old: bytes, new: bytes) -> int:
    """RFC 1624 eqn. 3 over the big-endian 16-bit words old -> new, every word included."""
    acc = ~hc & 0xFFFF
    for m, m2 in zip(_words(old), _words(new)):
        acc += (~m & 0xFFFF) + m2
    return ~fold(acc) & 0xFFFF


def rewrite_frame(f: bytes, table, slots: int, ttl_dec: int, ipver: int):
    """The translated frame, or None when frame f (its valid bit set) is not translated."""
    ihl = wellformed(f, ipver)
    if ihl is None:
        return None
    at_ttl = 8 if ipver == 4 else 7
    if not f[at_ttl] > ttl_dec:
        return None
    t = tuple_of(f, ipver, ihl)
    r = lookup(table, slots, t, ipver)
    if r is None:
        return None
    g = bytearray(f)
    g[at_ttl] = f[at_ttl] - ttl_dec
    a0 = 12 if ipver == 4 else 8
    na = len(t) - 4
    g[a0:a0 + na] = r[:na]
    g[ihl:ihl + 4] = r[na:]
    if ipver == 4:
        hc = update(int.from_bytes(f[10:12], "big"), bytes(f[8:10]) + t[:na], bytes(g[8:10]) + r[:na])
        g[10:12] = hc.to_bytes(2, "big")
    tc = update(int.from_bytes(f[ihl + 16:ihl + 18], "big"), t, r)
    g[ihl + 16:ihl + 18] = tc.to_bytes(2, "big")
    return bytes(g)


def rewrite(buf, offsets, valid, table, slots: int, ttl_dec: int, ipver: int):
    """(new_buf, hit): the whole buffer after the device call and n booleans, frame i translated."""
    buf = np.asarray(buf, np.uint8)
    offsets = np.asarray(offsets, np.uint64)
    n = offsets.size - 1
    ok = _gro.valid_bits(valid, n)
    out, hit = buf.copy(), np.zeros(n, bool)
    for i in range(n):
        if not ok[i]:
            continue
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        g = rewrite_frame(buf[o0:o1].tobytes(), table, slots, ttl_dec, ipver)
        if g is not None:
            out[o0:o1] = np.frombuffer(g, np.uint8)
            hit[i] = True
    return out, hit


# ---------------------------------------------------------------- test material
def frames(rng, ipver: int, pays, opts=None, ttl=None):
    """Valid frames of the transmit pass's model (tests/_tx.py), one per payload length, as a list of bytes; ttl: one
    value or one per frame (default random 1..255)."""
    import _tx
    c = _tx.Case(rng, ipver, [int(p) for p in pays], opts=opts)
    c.ip["ttl"][:] = rng.integers(1, 256, c.n) if ttl is None else ttl
    return _gro.case_frames(c)


def with_ip_options(f: bytes, ihl_words: int, rng) -> bytes:
    """An IPv4 frame with IHL 5 given ihl_words*4 - 20 random IP option bytes, lengths and checksums re-fixed."""
    extra = rng.integers(0, 256, ihl_words * 4 - 20, dtype=np.uint8).tobytes()
    g = bytearray(f[:20] + extra + f[20:])
    g[0] = 0x40 | ihl_words
    g[2:4] = len(g).to_bytes(2, "big")
    return _gro.refix(g, 4)


def random_tuples(rng, k: int, ipver: int):
    return [rng.integers(0, 256, TUPLE[ipver], dtype=np.uint8).tobytes() for _ in range(k)]


def chain_tuples(rng, ipver: int, k: int, home: int, slots: int):
    """k different tuples whose home slot is `home`: random addresses, the ports chosen with FL.ports_for_key."""
    out = []
    for j in range(k):
        a = rng.integers(0, 256, TUPLE[ipver] - 4, dtype=np.uint8).tobytes()
        st = FL.FNV_BASIS
        for q in range(0, len(a), 4):
            st = FL._mix(st, int.from_bytes(a[q:q + 4], "little"))
        k32 = (int(rng.integers(0, 1 << 32)) & ~(slots - 1) & 0xFFFFFFFF) | home
        t = a + FL.ports_for_key(st, k32).to_bytes(4, "little")
        assert key(t) & (slots - 1) == home
        out.append(t)
    assert len(set(out)) == k
    return out


def with_tuple(f: bytes, ipver: int, t: bytes) -> bytes:
    """Frame f with its addresses and ports replaced by tuple t, checksums re-fixed."""
    g = bytearray(f)
    ihl = (g[0] & 15) * 4 if ipver == 4 else 40
    a0, na = (12 if ipver == 4 else 8), len(t) - 4
    g[a0:a0 + na] = t[:na]
    g[ihl:ihl + 4] = t[na:]
    return _gro.refix(g, ipver)


def pack(fr, lead: int = 0, tail: int = 3, fill: int = FILL):
    """Frames packed back to back behind `lead` fill bytes, `tail` fill bytes after: (buf, offsets)."""
    offs = np.zeros(len(fr) + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in fr]) if fr else []
    offs += np.uint64(lead)
    return np.frombuffer(bytes([fill]) * lead + b"".join(fr) + bytes([fill]) * tail, np.uint8).copy(), offs
