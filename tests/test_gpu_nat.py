"""The in-place NAT rewrite on the GPU (nsx_nat_ipv4_tcp_rewrite_dev / nsx_nat_ipv6_tcp_rewrite_dev): the WHOLE
buffer — gaps, lead bytes, untranslated frames and a guard region on either side of it, all over a fill byte — and
the hit mask, bit-exact against the numpy restatement tests/_nat.py (held to the transmit pass's model by tests/test_nat_abi.py).
No case feeds a table without an empty entry: that the probe is a counted loop is checked by reading the kernel and
by the restatement (tests/test_nat_abi.py test_lookup_is_total)."""
import copy

import numpy as np
import pytest

import _gro
import _nat
import _rx
import _tx
from _gpu import dev, host, mask_words, setup_gpu, torch, nsx
from _gro_gpu import d as _d

pytestmark = pytest.mark.gpu

FILL = _nat.FILL
GUARD = 64        # fill bytes on either side of the buffer handed to the call, inside one device allocation
HIT_FILL = 0x5C   # the hit words (and one word past them) before the call


def setup_module(module):
    setup_gpu()


def _fn(ipver):
    return nsx.nat_ipv4_tcp_rewrite_dev if ipver == 4 else nsx.nat_ipv6_tcp_rewrite_dev


def _d64(a):
    return dev(np.ascontiguousarray(a, np.uint64).view(np.int64))


def _arena(buf):
    """buf between two guard regions in one allocation: (the arena, the view the call gets)."""
    arena = torch.full((GUARD + buf.size + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    view = arena[GUARD:GUARD + buf.size]
    view.copy_(dev(buf))
    return arena, view


def _valid_words(valid, n):
    w = mask_words(_gro.valid_bits(valid, n).astype(np.uint8))
    return _d64(w if w.size else np.zeros(1, np.uint64))


def _run(buf, offs, valid, table, slots, ttl_dec, ipver, d_valid=None):
    """One device call: (arena bytes, hit words incl. one guard word) on the host."""
    n = offs.size - 1
    words = (n + 63) // 64
    arena, view = _arena(buf)
    hit = torch.full((8 * (words + 1),), HIT_FILL, dtype=torch.uint8, device="cuda").view(torch.int64)
    d_valid = _valid_words(valid, n) if d_valid is None else d_valid
    res = _fn(ipver)(view, _d64(offs), d_valid, dev(table), slots, ttl_dec=ttl_dec, hit=hit)
    assert res is hit
    return host(arena), host(hit).view(np.uint64)


def _want(buf, offs, valid, table, slots, ttl_dec, ipver):
    n = offs.size - 1
    out, hit = _nat.rewrite(buf, offs, valid, table, slots, ttl_dec, ipver)
    guard = np.full(GUARD, FILL, np.uint8)
    words = np.concatenate([mask_words(hit.astype(np.uint8)).reshape(-1),
                            np.full(8, HIT_FILL, np.uint8).view(np.uint64)])
    assert words.size == (n + 63) // 64 + 1
    return np.concatenate([guard, out, guard]), words, hit


def _check(buf, offs, valid, table, slots, ttl_dec, ipver, what="", d_valid=None):
    """The whole arena and the hit words against the model; returns the model's hit booleans."""
    got, ghit = _run(buf, offs, valid, table, slots, ttl_dec, ipver, d_valid=d_valid)
    want, whit, hit = _want(buf, offs, valid, table, slots, ttl_dec, ipver)
    if not np.array_equal(ghit, whit):
        at = np.nonzero(ghit != whit)[0]
        raise AssertionError(f"{what}: hit word {at[0]}: got {ghit[at[0]]:#018x}, want {whit[at[0]]:#018x}")
    if not np.array_equal(got, want):
        d = np.nonzero(got != want)[0]
        b = int(d[0]) - GUARD
        i = int(np.searchsorted(offs, np.uint64(max(b, 0)), side="right")) - 1
        raise AssertionError(f"{what}: {d.size} bytes differ, first at buffer byte {b} (frame {i}, its byte "
                             f"{b - int(offs[max(i, 0)])}): got {got[d[:8]]}, want {want[d[:8]]}")
    return hit


def _rules(rng, fr, ipver, ratio=1.0, extra=0, sparse=1):
    """A table with a rule for a share `ratio` of the well-formed frames' tuples (new tuples random) and `extra`
    rules no frame matches, of `sparse` times the smallest size: (table, slots). Built by tests/_nat.build_table,
    which tests/test_nat_abi.py holds to nsx_nat_table_build_host byte for byte."""
    ts = []
    for f in fr:
        ihl = _nat.wellformed(f, ipver)
        if ihl is not None and rng.random() < ratio:
            ts.append(_nat.tuple_of(f, ipver, ihl))
    match = list(dict.fromkeys(ts + _nat.random_tuples(rng, extra, ipver)))
    slots = sparse * nsx.nat_table_slots(len(match))
    return _nat.build_table(ipver, match, _nat.random_tuples(rng, len(match), ipver), slots), slots


# ---------------------------------------------------------------- alignment: no store leaves the frame
KINDS = [(4, "minimal"), (4, "odd"), (4, "ihl6"), (4, "ihl15"), (6, "minimal"), (6, "odd")]


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("ipver,kind", KINDS, ids=[f"v{v}-{k}" for v, k in KINDS])
def test_packed_frames_at_every_alignment(ipver, kind, lead):
    """150 frames packed densely behind 0-3 lead bytes, the last one ending exactly at the buffer's end: minimal
    frames (40-byte IPv4, 60-byte IPv6: TCP byte 17 is 3 bytes from the neighbour), odd lengths (every alignment in
    one batch), IPv4 with IHL 6 and IHL 15. Two frames in three are translated; their neighbours must not change."""
    rng = np.random.default_rng(0x7A1 + 8 * lead + ipver + len(kind))
    n = 150
    pays = np.zeros(n, int) if kind == "minimal" else \
        rng.integers(0, 40, n) * 2 + 1 if kind == "odd" else rng.integers(0, 9, n)
    fr = _nat.frames(rng, ipver, pays)
    if kind.startswith("ihl"):
        fr = [_nat.with_ip_options(f, int(kind[3:]), rng) for f in fr]
        assert all(_nat.wellformed(f, 4) == 4 * int(kind[3:]) for f in fr)
    buf, offs = _nat.pack(fr, lead=lead, tail=0)
    assert int(offs[-1]) == buf.size
    table, slots = _rules(rng, fr, ipver, ratio=0.67, extra=5)
    hit = _check(buf, offs, np.ones(n, bool), table, slots, 1, ipver, what=f"{kind} lead {lead}")
    assert 60 < hit.sum() < 140


# ---------------------------------------------------------------- n across wave and block edges
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 3000])
@pytest.mark.parametrize("ipver", [4, 6])
def test_frame_counts_across_wave_and_block_edges(ipver, n):
    """The hit words, the word past them included: bits past n are 0, no word past ceil(n/64) is written (n = 0
    writes none), the last lanes of the last wave and block do their frames."""
    rng = np.random.default_rng(0x7B1 + n + ipver)
    fr = _nat.frames(rng, ipver, rng.integers(0, 30, n)) if n else []
    buf, offs = _nat.pack(fr, lead=n % 4)
    table, slots = _rules(rng, fr, ipver, extra=3)
    valid = rng.random(n) < 0.9
    valid[-1:] = True
    hit = _check(buf, offs, valid, table, slots, 0, ipver, what=f"n {n}")
    assert np.array_equal(hit, valid)


# ---------------------------------------------------------------- TTL
@pytest.mark.parametrize("ttl_dec", [0, 1, 255])
@pytest.mark.parametrize("ipver", [4, 6])
def test_ttl_edges(ipver, ttl_dec):
    """TTL / hop limit equal to ttl_dec (not translated), ttl_dec + 1 (becomes 1), 255, 0 and 1; every tuple is in
    the table."""
    rng = np.random.default_rng(0x7C1 + ttl_dec + ipver)
    ttls = np.resize(np.array([ttl_dec, min(ttl_dec + 1, 255), 255, 0, 1, 128], np.uint8), 96)
    fr = _nat.frames(rng, ipver, rng.integers(0, 20, ttls.size), ttl=ttls)
    buf, offs = _nat.pack(fr, lead=3)
    table, slots = _rules(rng, fr, ipver)
    hit = _check(buf, offs, np.ones(ttls.size, bool), table, slots, ttl_dec, ipver, what=f"ttl_dec {ttl_dec}")
    assert np.array_equal(hit, ttls > ttl_dec)


# ---------------------------------------------------------------- carries
def _ones_add(a, b):
    s = a + b
    return (s & 0xFFFF) + (s >> 16)


def _zero_checksum(f: bytes, ipver: int, which: str) -> bytes:
    """Frame f (valid) changed in a word its checksum covers — the IPv4 ident, or the last whole payload word — so
    that the checksum field (which: "ip" or "tcp") becomes 0x0000 and still verifies."""
    g = bytearray(f)
    ihl = (g[0] & 15) * 4 if ipver == 4 else 40
    at_field, at_word = (10, 4) if which == "ip" else (ihl + 16, ihl + 20 + ((len(g) - ihl - 20) // 2 - 1) * 2)
    field, word = int.from_bytes(g[at_field:at_field + 2], "big"), int.from_bytes(g[at_word:at_word + 2], "big")
    g[at_word:at_word + 2] = _ones_add(word, field).to_bytes(2, "big")  # sum + ~sum = 0xFFFF: the field becomes 0
    g = bytearray(_gro.refix(g, ipver))
    assert g[at_field:at_field + 2] == b"\0\0"
    return bytes(g)


@pytest.mark.parametrize("ipver", [4, 6])
def test_carry_edges(ipver):
    """Tuples of all 0x00 and all 0xFF bytes turned into each other and into random ones (every ~m and m' of 0x0000
    and 0xFFFF); checksum fields that are 0x0000 on entry; TCP and IPv4 header checksums that are wrong while the
    valid bit is set — the model keeps the error, so must the kernel."""
    rng = np.random.default_rng(0x7D1 + ipver)
    tb = _nat.TUPLE[ipver]
    zero, ff = bytes(tb), b"\xff" * tb
    half = bytes(tb - 4) + b"\xff" * 4
    rnd = _nat.random_tuples(rng, 4, ipver)
    match = [zero, ff, half, rnd[0], rnd[1]]
    new = [ff, zero, zero, ff, rnd[2]]
    base = _nat.frames(rng, ipver, [8, 9, 10, 11, 12, 13, 14, 15], ttl=64)
    fr = [_nat.with_tuple(f, ipver, match[i % 5]) for i, f in enumerate(base)]
    fr += [_zero_checksum(_nat.with_tuple(base[i], ipver, match[i]), ipver, "tcp") for i in range(5)]
    if ipver == 4:
        fr += [_zero_checksum(_nat.with_tuple(base[i], ipver, match[i]), ipver, "ip") for i in range(5)]
    ihl = 20 if ipver == 4 else 40
    for i in range(5):  # wrong checksums, by one bit and by the whole field
        for at, flip in ((ihl + 16, 0x01), (ihl + 17, 0xFF)) + (((10, 0x80), (11, 0xFF)) if ipver == 4 else ()):
            g = bytearray(_nat.with_tuple(base[i + 1], ipver, match[i]))
            g[at] ^= flip
            fr.append(bytes(g))
    table = _nat.build_table(ipver, match, new, 16)
    for lead in (0, 1):
        buf, offs = _nat.pack(fr, lead=lead)
        hit = _check(buf, offs, np.ones(len(fr), bool), table, 16, 1, ipver, what=f"carry lead {lead}")
        assert hit.all()


# ---------------------------------------------------------------- mixed batches
def _mixed(rng, ipver, n, lead):
    kinds = _rx.KINDS if ipver == 4 else _rx.KINDS6
    buf, offs, ks = _rx.batch(rng, n, kinds=kinds, lead=lead, max_payload=120, ip=ipver)
    fr = [buf[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]
    return buf, offs, ks, fr


@pytest.mark.parametrize("ipver", [4, 6])
def test_mixed_batch_with_every_valid_bit_set(ipver):
    """Every kind of frame the receive pass distinguishes (malformed, fragments, non-TCP, bad sums), all valid bits
    set: the malformed ones are untouched whatever the table says, the well-formed ones with bad sums keep their
    error."""
    rng = np.random.default_rng(0x7E1 + ipver)
    n = 1500
    buf, offs, ks, fr = _mixed(rng, ipver, n, lead=1)
    table, slots = _rules(rng, fr, ipver, ratio=0.9, extra=20)
    hit = _check(buf, offs, np.ones(n, bool), table, slots, 1, ipver, what="mixed, all bits set")
    wf = np.array([_nat.wellformed(f, ipver) is not None for f in fr])
    assert not hit[~wf].any() and 0 < (~wf).sum() and hit.sum() > n // 4


@pytest.mark.parametrize("ipver", [4, 6])
def test_mixed_batch_with_the_receive_pass_mask(ipver):
    """The same kind of batch with the mask the GPU receive pass gives for it, handed over without leaving the
    device: only frames that verify are translated."""
    rng = np.random.default_rng(0x7F1 + ipver)
    n = 1500
    buf, offs, ks, fr = _mixed(rng, ipver, n, lead=2)
    table, slots = _rules(rng, fr, ipver, ratio=0.9, extra=20)
    rx = nsx.rx_ipv4_tcp_verify_dev if ipver == 4 else nsx.rx_ipv6_tcp_verify_dev
    d_mask = rx(dev(buf), _d64(offs))
    valid = _gro.valid_bits(host(d_mask).view(np.uint64), n)
    assert 0 < valid.sum() < n
    hit = _check(buf, offs, valid, table, slots, 1, ipver, what="mixed, true mask", d_valid=d_mask)
    assert not hit[~valid].any() and hit.sum() > n // 8


# ---------------------------------------------------------------- table shapes
@pytest.mark.parametrize("ipver", [4, 6])
def test_table_shapes(ipver):
    """Misses only; n_rules = 0; slots = 16 with 8 rules; a collision chain of 4 with the hit last; a chain that
    wraps past the last slot; a rule whose new tuple equals its match tuple."""
    rng = np.random.default_rng(0x801 + ipver)
    n = 200
    base = _nat.frames(rng, ipver, rng.integers(0, 25, n))
    ones = np.ones(n, bool)
    buf, offs = _nat.pack(base, lead=1)
    # misses: a full-sized table none of whose rules matches; and no rules at all
    table, slots = _rules(rng, [], ipver, extra=100)
    assert not _check(buf, offs, ones, table, slots, 1, ipver, what="misses").any()
    assert not _check(buf, offs, ones, _nat.build_table(ipver, [], [], 16), 16, 1, ipver, what="no rules").any()
    # slots = 16, half full
    match = [_nat.tuple_of(f, ipver) for f in base[:8]]
    table = _nat.build_table(ipver, match, _nat.random_tuples(rng, 8, ipver), 16)
    assert _check(buf, offs, ones, table, 16, 0, ipver, what="16 slots").sum() == 8
    # chains: every frame carries one of the chain's tuples; also the tuple of a fifth, absent chain member (a miss
    # that walks the whole chain)
    for home, slots, what in ((5, 64, "chain"), (14, 16, "wrapping chain")):
        chain = _nat.chain_tuples(rng, ipver, 5, home=home, slots=slots)
        fr = [_nat.with_tuple(f, ipver, chain[i % 5]) for i, f in enumerate(base)]
        new = _nat.random_tuples(rng, 4, ipver)
        table = _nat.build_table(ipver, chain[:4], new, slots)
        assert [_nat._entry(table, (home + j) % slots, ipver)[1] for j in range(4)] == chain[:4]
        buf2, offs2 = _nat.pack(fr, lead=2)
        hit = _check(buf2, offs2, ones, table, slots, 0, ipver, what=what)
        assert np.array_equal(hit, np.arange(n) % 5 != 4)
        last = np.arange(n) % 5 == 3  # the hit is the chain's last entry
        assert all(_nat.lookup(table, slots, _nat.tuple_of(fr[i], ipver), ipver) == new[3] for i in np.nonzero(last)[0])
    # identity rules: only the TTL and the checksum over it change
    match = [_nat.tuple_of(f, ipver) for f in base[:50]]
    table = _nat.build_table(ipver, match, match, 128)
    assert _check(buf, offs, ones, table, 128, 3, ipver, what="identity").sum() > 40


# ---------------------------------------------------------------- closure on the device
@pytest.mark.parametrize("ipver", [4, 6])
def test_closure_with_the_transmit_and_receive_passes(ipver):
    """nsx_tx_*_build_dev -> nsx_rx_*_verify_dev -> rewrite -> nsx_rx_*_verify_dev without leaving the device: the
    mask after is the mask before (frames broken before the first verify stay broken and untouched), and the buffer
    equals what nsx_tx_*_build_dev builds from the translated fields."""
    rng = np.random.default_rng(0x811 + ipver)
    n, ttl_dec = 600, 2
    c = _tx.Case(rng, ipver, rng.integers(0, 30, n) * 4)  # frame lengths are multiples of 4: the slots are dense
    c.ip["ttl"][:] = rng.integers(0, 6, n)
    off = c.packed()
    assert np.array_equal(np.diff(off), c.flen)
    build = nsx.tx_ipv4_tcp_build_dev if ipver == 4 else nsx.tx_ipv6_tcp_build_dev
    rx = nsx.rx_ipv4_tcp_verify_dev if ipver == 4 else nsx.rx_ipv6_tcp_verify_dev
    iph = _tx.IPH[ipver]
    broken = np.arange(n) % 11 == 0

    def built(case):
        ip = {k: _d(v.reshape(-1)) for k, v in case.ip.items()}
        fields = {k: _d(v) for k, v in case.fields.items()}
        out = torch.full((int(off[-1]),), FILL, dtype=torch.uint8, device="cuda")
        build(ip, fields, _d(case.data), _d64(case.data_off), out, _d64(off))
        at = torch.from_numpy((off[:-1][broken] + np.uint64(iph + 19)).astype(np.int64)).cuda()
        out[at] ^= 0x10  # the urgent pointer's low byte: the TCP checksum no longer verifies
        return out

    d_buf, d_off = built(c), _d64(off)
    before = rx(d_buf, d_off).clone()
    frames0 = host(d_buf)
    fr = [frames0[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]
    table, slots = _rules(rng, fr, ipver, ratio=0.8)
    d_hit = _fn(ipver)(d_buf, d_off, before, dev(table), slots, ttl_dec=ttl_dec)
    after = rx(d_buf, d_off)
    valid = _gro.valid_bits(host(before).view(np.uint64), n)
    assert np.array_equal(valid, ~broken) and np.array_equal(host(after), host(before))
    hit = _gro.valid_bits(host(d_hit).view(np.uint64), n)
    want_hit = np.array([valid[i] and c.ip["ttl"][i] > ttl_dec and
                         _nat.lookup(table, slots, _nat.tuple_of(fr[i], ipver), ipver) is not None for i in range(n)])
    assert np.array_equal(hit, want_hit) and 100 < hit.sum() < n
    c2 = copy.deepcopy(c)
    alen = 4 if ipver == 4 else 16
    for i in np.nonzero(hit)[0]:
        t = _nat.lookup(table, slots, _nat.tuple_of(fr[i], ipver), ipver)
        c2.ip["src"][i], c2.ip["dst"][i] = np.frombuffer(t[:alen], np.uint8), np.frombuffer(t[alen:2 * alen], np.uint8)
        c2.fields["src_port"][i] = int.from_bytes(t[2 * alen:2 * alen + 2], "big")
        c2.fields["dst_port"][i] = int.from_bytes(t[2 * alen + 2:], "big")
        c2.ip["ttl"][i] -= ttl_dec
    assert np.array_equal(host(d_buf), host(built(c2)))


# ---------------------------------------------------------------- random family
@pytest.mark.parametrize("seed", range(10))
def test_random_batches(seed):
    """~2000 frames per seed and IP version: random kinds (malformed among them), lead bytes, hit ratio, table load,
    ttl_dec, and a random valid mask."""
    for ipver in (4, 6):
        rng = np.random.default_rng(0x900 + 2 * seed + ipver)
        n = int(rng.integers(1800, 2200))
        buf, offs, ks, fr = _mixed(rng, ipver, n, lead=int(rng.integers(0, 4)))
        table, slots = _rules(rng, fr, ipver, ratio=float(rng.random()), extra=int(rng.integers(0, 200)),
                              sparse=int(rng.choice([1, 1, 4])))
        valid = rng.random(n) < rng.random()
        _check(buf, offs, valid, table, slots, int(rng.choice([0, 1, 2, 64, 255])), ipver, what=f"seed {seed} v{ipver}")


# ---------------------------------------------------------------- graph capture
@pytest.mark.parametrize("ipver", [4, 6])
def test_graph_capture_and_replay(ipver):
    """The call captured into a torch.cuda.graph runs nothing at capture and rewrites the buffer on replay."""
    rng = np.random.default_rng(0x821 + ipver)
    n = 300
    fr = _nat.frames(rng, ipver, rng.integers(0, 40, n))
    buf, offs = _nat.pack(fr, lead=1)
    table, slots = _rules(rng, fr, ipver, ratio=0.7)
    valid = np.ones(n, bool)
    want, whit, _ = _want(buf, offs, valid, table, slots, 1, ipver)
    arena, view = _arena(buf)
    d_offs, d_valid, d_table = _d64(offs), _valid_words(valid, n), dev(table)
    hit = torch.full((8 * (whit.size),), HIT_FILL, dtype=torch.uint8, device="cuda").view(torch.int64)
    # a first call outside capture (library and device-info setup), on a copy of the buffer
    _fn(ipver)(view.clone(), d_offs, d_valid, d_table, slots, ttl_dec=1)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        _fn(ipver)(view, d_offs, d_valid, d_table, slots, ttl_dec=1, hit=hit)
    torch.cuda.synchronize()
    assert np.array_equal(host(view), buf) and (host(hit).view(np.uint8) == HIT_FILL).all()  # capture ran nothing
    g.replay()
    assert np.array_equal(host(arena), want) and np.array_equal(host(hit).view(np.uint64), whit)
