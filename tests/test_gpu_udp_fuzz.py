"""Seeded random batches for the UDP passes against the CPU restatement tests/_udp.py: transmit, segmentation offload,
and the receive verify over built frames with random corruptions. The GPU families are marked `gpu`; the unmarked
tests check the generator itself on any host — it is a pure function of its case number, and over the seeds used it
draws every corruption class, both IP versions, every flag / NULL-member choice and every launch shape."""
import numpy as np
import pytest

import _udp

TX_CASES, USO_CASES, RX_CASES = 24, 24, 24
NULLABLE = ("ident", "ttl", "tclass", "flow")
TUNES = (None, dict(blocks_per_cu=1, run_segs=1), dict(blocks_per_cu=1, run_segs=3), dict(blocks_per_cu=2, run_segs=64),
         dict(run_segs=16))
GSO = (1, 2, 7, 8, 100, 512, 1200, 1472, 9000)
FILL = 0xAB


def _lens(rng, n):
    """n payload lengths of one of four profiles: tiny, small datagrams, MTU-sized, anything up to a few rows."""
    profile = int(rng.integers(4))
    if profile == 0:
        return rng.integers(0, 20, n)
    if profile == 1:
        return rng.integers(32, 73, n)
    if profile == 2:
        return rng.integers(1200, 1473, n)
    return rng.integers(0, 4200, n)


def _gaps(rng, off):
    """Slots with 0-32 spare bytes behind some of them, the first slot 0-16 bytes into the buffer."""
    n = off.size - 1
    g = np.zeros(n + 1, np.uint64)
    g[1:] = np.cumsum(np.diff(off) + (rng.integers(0, 9, n) * 4 * (rng.integers(0, 3, n) == 0)).astype(np.uint64))
    return g + np.uint64(4 * int(rng.integers(5)))


def _choices(rng, ipver, case):
    flags = _udp.NO_CSUM if ipver == 4 and case % 6 == 0 else 0
    null = tuple(k for k in NULLABLE if rng.integers(4) == 0)
    return flags, null, int(rng.integers(len(TUNES))), bool(rng.integers(2))


def tx_batch(case):
    """(Case, off, flags, null, tune index, want_raw): 100-500 frames behind 0-3 lead bytes."""
    rng = np.random.default_rng(0x7D0000 + case)
    ipver = 4 if case % 2 == 0 else 6
    n = int(rng.integers(100, 501))
    c = _udp.Case(rng, ipver, _lens(rng, n), lead=int(rng.integers(4)))
    for i in rng.choice(n, 3, replace=False):  # a few frames whose computed checksum is 0
        if int(c.plen[i]) >= 3:
            _udp.craft_ffff(c, int(i), int(rng.integers(int(c.plen[i]) - 1)))
    off = c.packed() if rng.integers(2) else _gaps(rng, c.packed())
    return (c, off) + _choices(rng, ipver, case)


def uso_batch(case):
    """(Batch, off, flags, null, tune index, want_raw): super-datagrams of one gso class (a quarter of them with a gso
    of their own between half and twice that), a few hundred frames."""
    rng = np.random.default_rng(0x7D1000 + case)
    ipver = 4 if case % 2 == 0 else 6
    gso = GSO[case % len(GSO)]
    want = int(rng.integers(100, 501))
    n = max(2, want // 6)
    lens = np.minimum(rng.integers(0, 12 * gso + 1, n), 60000)
    lens[rng.choice(n, 2, replace=False)] = (0, gso)
    g = np.where(rng.integers(0, 4, n) == 0, rng.integers((gso + 1) // 2, 2 * gso + 1, n), gso)
    b = _udp.Batch(rng, ipver, lens, g, lead=int(rng.integers(4)))
    b.sup.ip["ident"][rng.integers(0, n, 2)] = 0xFFFE
    off = b.off if rng.integers(2) else _gaps(rng, b.off)
    return (b, off) + _choices(rng, ipver, case)


def rx_batch(case):
    """(ipver, buf, offs, kinds, tune index): 100-500 built frames, about a third of them corrupted, one kind each,
    behind 0-3 junk lead bytes."""
    rng = np.random.default_rng(0x7D2000 + case)
    ipver = 4 if case % 2 == 0 else 6
    n = int(rng.integers(100, 501))
    c = _udp.Case(rng, ipver, _lens(rng, n), lead=int(rng.integers(4)))
    fr, _ = _udp.frames(c, flags=_udp.NO_CSUM if ipver == 4 and case % 8 == 0 else 0)
    kinds = []
    for i in range(n):
        kind = _udp.CORRUPTIONS[int(rng.integers(1, len(_udp.CORRUPTIONS)))] if rng.integers(3) == 0 else "none"
        fr[i] = _udp.corrupt(rng, fr[i], ipver, kind)
        kinds.append(kind)
    buf, offs = _udp.concat(fr, lead=int(rng.integers(4)), rng=rng)
    return ipver, buf, offs, kinds, int(rng.integers(len(TUNES)))


# ---------------------------------------------------------------- the generator, on any host
def test_generators_are_deterministic():
    for gen, cases in ((tx_batch, (0, 1, 7)), (uso_batch, (0, 1, 8)), (rx_batch, (0, 1, 9))):
        for k in cases:
            a, b = gen(k), gen(k)
            if gen is rx_batch:
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3:] == b[3:]
                continue
            ca, cb = (a[0], b[0]) if gen is tx_batch else (a[0].sup, b[0].sup)
            assert np.array_equal(ca.data, cb.data) and np.array_equal(ca.data_off, cb.data_off)
            assert all(np.array_equal(ca.ip[f], cb.ip[f]) for f in ca.ip) and np.array_equal(a[1], b[1])
            assert a[2:] == b[2:]
            if gen is uso_batch:
                assert np.array_equal(a[0].gso, b[0].gso) and np.array_equal(a[0].first, b[0].first)


def test_generators_cover_every_class():
    """Over the seeds used: every corruption class on both IP versions, with verdicts that are not all one value;
    NO_CSUM, every NULL member, d_udp_raw NULL, gaps and every launch shape for tx and USO; crafted 0xFFFF frames;
    every gso class, idents that wrap, empty super-datagrams and cuts that leave a short last frame."""
    seen = {4: set(), 6: set()}
    for k in range(RX_CASES):
        ipver, buf, offs, kinds, _ = rx_batch(k)
        seen[ipver] |= set(kinds)
        valid, _, _ = _udp.rx_expected(ipver, buf, offs)
        none = np.array([x == "none" for x in kinds])
        assert valid[none].all() and 100 <= len(kinds) <= 500
        no_csum = ipver == 4 and k % 8 == 0  # the field is 0: IPv4 accepts the datagram whatever its bytes sum to
        assert no_csum or not valid[np.array([x == "payload_byte" for x in kinds])].any()
        assert not valid[np.array([x in ("udp_len_short", "udp_len_long", "protocol", "length_field",
                                         "truncate", "version") for x in kinds])].any()
        assert valid[np.array([x == "padding" for x in kinds])].all()
        assert (valid[np.array([x.startswith("field_zero") for x in kinds])] == (ipver == 4)).all()
    assert seen[4] == seen[6] == set(_udp.CORRUPTIONS)
    for gen, cases in ((tx_batch, TX_CASES), (uso_batch, USO_CASES)):
        flags, nulls, tunes, raws, gaps, ffff, short = set(), set(), set(), set(), set(), 0, False
        for k in range(cases):
            x, off, fl, null, tune, want_raw = gen(k)
            c = x if gen is tx_batch else _udp.expand(x)
            flags.add((c.ipver, fl))
            nulls |= set(null)
            tunes.add(tune)
            raws.add(want_raw)
            gaps.add(bool((np.diff(off) != ((c.flen + np.uint64(3)) & ~np.uint64(3))).any()))
            _, wraw = _udp.frames(c)
            ffff += int((wraw == 0xFFFF).sum())
            assert 50 <= c.n <= 2500
            if gen is uso_batch:
                assert (x.sup.plen == 0).any() and (np.diff(x.first) > 1).any()
                short |= bool(((c.plen > 0) & (c.plen < x.gso[x.seg])).any())
        assert flags == {(4, 0), (4, 1), (6, 0)} and nulls == set(NULLABLE) and tunes == set(range(len(TUNES)))
        assert raws == {True, False} and gaps == {True, False}
        assert ffff >= 10 if gen is tx_batch else short
    assert {GSO[k % len(GSO)] for k in range(USO_CASES)} == set(GSO)


# ---------------------------------------------------------------- the GPU families
def _gpu():
    import _gpu
    _gpu.setup_gpu()
    return _gpu


_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
           np.dtype(np.uint64): np.int64}


def _d(G, a):
    a = np.ascontiguousarray(a)
    return G.dev(a.view(_SIGNED[a.dtype]))


def _check(G, off, out, raw, want, wraw, what):
    if raw is not None:
        got = G.u16(raw)
        bad = np.nonzero(got != wraw)[0]
        assert bad.size == 0, (what, bad[:8], got[bad[:8]], wraw[bad[:8]])
    got = G.host(out)
    if not np.array_equal(got, want):
        d = np.nonzero(got != want)[0]
        i = int(np.searchsorted(np.asarray(off, np.uint64), d[0], side="right")) - 1
        raise AssertionError(f"{what}: {d.size} bytes differ, first at {d[0]} (frame {i}): got {got[d[:8]]}, want "
                             f"{want[d[:8]]}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(TX_CASES))
def test_fuzz_udp_tx(case):
    G = _gpu()
    c, off, flags, null, tune, want_raw = tx_batch(case)
    total = int(off[-1]) + 8
    want, wraw = _udp.expected(c, off, fill=FILL, flags=flags, null=null, total=total)
    out = G.torch.full((total,), FILL, dtype=G.torch.uint8, device="cuda")
    raw = G.torch.full((c.n,), 0x5A5A, dtype=G.torch.int16, device="cuda") if want_raw else None
    fn = G.nsx.udp_tx_ipv4_build_dev if c.ipver == 4 else G.nsx.udp_tx_ipv6_build_dev
    fn({k: _d(G, v.reshape(-1)) for k, v in c.ip.items() if k not in null}, {k: _d(G, v) for k, v in c.ports.items()},
       _d(G, c.data), _d(G, c.data_off), out, _d(G, off), flags=flags, raw=raw, tune=TUNES[tune])
    _check(G, off, out, raw, want, wraw, f"tx case {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(USO_CASES))
def test_fuzz_udp_uso(case):
    G = _gpu()
    b, off, flags, null, tune, want_raw = uso_batch(case)
    total = int(off[-1]) + 8
    want, wraw, _ = _udp.uso_expected(b, off=off, fill=FILL, flags=flags, null=null, total=total)
    out = G.torch.full((total,), FILL, dtype=G.torch.uint8, device="cuda")
    raw = G.torch.full((b.nf,), 0x5A5A, dtype=G.torch.int16, device="cuda") if want_raw else None
    s = b.sup
    fn = G.nsx.udp_uso_ipv4_build_dev if b.ipver == 4 else G.nsx.udp_uso_ipv6_build_dev
    fn({k: _d(G, v.reshape(-1)) for k, v in s.ip.items() if k not in null}, {k: _d(G, v) for k, v in s.ports.items()},
       _d(G, s.data), _d(G, s.data_off), _d(G, b.gso), _d(G, b.first), _d(G, b.seg), out, _d(G, off), flags=flags,
       raw=raw, tune=TUNES[tune])
    _check(G, off, out, raw, want, wraw, f"uso case {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(RX_CASES))
def test_fuzz_udp_rx(case):
    G = _gpu()
    ipver, buf, offs, kinds, tune = rx_batch(case)
    n = len(kinds)
    valid, wipr, wudr = _udp.rx_expected(ipver, buf, offs)
    mask = G.torch.full(((n + 63) // 64,), 0x5A5A5A5A5A5A5A5A, dtype=G.torch.int64, device="cuda")
    ipr = G.torch.zeros(n, dtype=G.torch.int16, device="cuda")
    udr = G.torch.zeros(n, dtype=G.torch.int16, device="cuda")
    if ipver == 4:
        G.nsx.udp_rx_ipv4_verify_dev(G.dev(buf), _d(G, offs), mask=mask, ip_raw=ipr, udp_raw=udr, tune=TUNES[tune])
        bad = np.nonzero(G.u16(ipr) != wipr)[0]
        assert bad.size == 0, ("ip_raw", bad[:8], [kinds[i] for i in bad[:8]])
    else:
        G.nsx.udp_rx_ipv6_verify_dev(G.dev(buf), _d(G, offs), mask=mask, udp_raw=udr, tune=TUNES[tune])
    bad = np.nonzero(G.u16(udr) != wudr)[0]
    assert bad.size == 0, ("udp_raw", bad[:8], [kinds[i] for i in bad[:8]], G.u16(udr)[bad[:8]], wudr[bad[:8]])
    got = np.unpackbits(G.host(mask).view(np.uint8), bitorder="little").astype(bool)
    bad = np.nonzero(got[:n] != valid)[0]
    assert bad.size == 0, ("mask", bad[:8], [kinds[i] for i in bad[:8]])
    assert not got[n:].any()
