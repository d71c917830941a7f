"""Every device pass with offsets past 2^32 and a frame of about 2^32 bytes (tests/_far.py): one zeroed arena of
2^32 + 8 MiB bytes holds the near frames, the span's 256 defined bytes and the far frames at their device addresses;
every expected value comes from the project's models run on the compact twin, bit-exact. tests/test_far_layout.py shows
on the CPU that a kernel which kept only the low word of the span's length could not pass. Nothing of 4 GiB goes to the
host: after each call the defined ranges are compared with 64 guard bytes on either side and the rest of the arena is
checked by device reductions to be still zero."""
import numpy as np
import pytest

import _far
import _gro
import _gro_gpu
import _tso
import _tx
from _gpu import dev, host, mask_words, setup_gpu, torch, u16, nsx
from oracle import csum_oracle as O
from test_gpu_rx import PFX, TUNES

pytestmark = pytest.mark.gpu

RX_TUNES = [None] + TUNES + [t for t in PFX if t not in TUNES]
# Every receive launch walks the 4 GiB span on one wave (the streamed fallback of every form: a frame too long for a
# slot), about two thirds of a second, so the forms of one batch run as cases of four launches each.
RX_FORMS = [RX_TUNES[k:k + 4] for k in range(0, len(RX_TUNES), 4)]
_U = {"uint8": np.uint8, "int16": np.uint16, "int32": np.uint32, "int64": np.uint64}
_d = _gro_gpu.d
placements = pytest.mark.parametrize("placement", _far.PLACEMENTS, ids=_far.pid)
mixes = pytest.mark.parametrize("mix", _far.MIXES)


@pytest.fixture(scope="module")
def arena():
    setup_gpu()
    a = torch.zeros(_far.ARENA, dtype=torch.uint8, device="cuda")
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def gro_data():
    """nsx_gro_out.data at its worst-case extent, d_offsets[n] - d_offsets[0] bytes, every byte the fill."""
    setup_gpu()
    a = torch.full((_far.ARENA,), _gro_gpu.FILL, dtype=torch.uint8, device="cuda")
    yield a
    del a
    torch.cuda.empty_cache()


def _put(arena, pieces):
    """Zero the arena (one memset) and copy the defined pieces in."""
    arena.zero_()
    for d, b in pieces:
        if len(b):
            arena[d:d + len(b)].copy_(torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()))


def _all_equal(t, byte):
    """One device reduction: every byte of the uint8 tensor t is `byte` (8 bytes at a time over the aligned middle)."""
    n = t.numel()
    a = min((-t.data_ptr()) % 8, n)
    m = (n - a) // 8
    word = int.from_bytes(bytes([byte]) * 8, "little", signed=True)
    ok = bool((t[:a] == byte).all()) and bool((t[a + 8 * m:] == byte).all())
    return ok and (m == 0 or bool((t[a:a + 8 * m].view(torch.int64) == word).all()))


def _check_arena(arena, pieces, what=""):
    """The arena holds exactly `pieces`: each window (the pieces with their guard bytes) compared on the host, the
    slices between the windows still zero by a device reduction."""
    torch.cuda.synchronize()
    at = 0
    for lo, hi in _far.windows(pieces):
        assert _all_equal(arena[at:lo], 0), f"{what}: bytes written in [{at}, {lo}), outside every frame"
        got, want = arena[lo:hi].cpu().numpy(), _far.window_bytes(pieces, lo, hi)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            raise AssertionError(f"{what}: {bad.size} bytes differ in [{lo}, {hi}), first at {lo + int(bad[0])}: got "
                                 f"{got[bad[:8]]}, want {want[bad[:8]]}")
        at = hi
    assert _all_equal(arena[at:], 0), f"{what}: bytes written in [{at}, {_far.ARENA})"


def _offs(r):
    return dev(r.far_offs.view(np.int64))


# ------------------------------------------------------------------ the receive pass
@pytest.mark.parametrize("forms", range(len(RX_FORMS)))
@mixes
@placements
@pytest.mark.parametrize("ipver", [4, 6])
def test_far_rx_every_launch_form(arena, ipver, placement, mix, forms):
    """nsx_rx_ipv4_tcp_verify_dev / nsx_rx_ipv6_tcp_verify_dev: mask and raw sums of every frame — the span (not
    well-formed: longer than any length field can say, whatever its low word and its head say), the frame across
    byte 2^32 and every frame above it — in the default launch and every forced form of tests/test_gpu_rx.py."""
    r = _far.rx_batch(ipver, placement, mix)
    want = _far.rx_model(ipver, r.buf, r.offs)
    _put(arena, r.pieces())
    offs = _offs(r)
    names = ("mask", "ip_raw", "tcp_raw") if ipver == 4 else ("mask", "tcp_raw")
    for tune in RX_FORMS[forms]:
        mask = torch.full(((r.n + 63) // 64,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
        ipr = torch.full((r.n,), 0x5A5A, dtype=torch.int16, device="cuda")
        tcpr = torch.full((r.n,), 0x5A5A, dtype=torch.int16, device="cuda")
        if ipver == 4:
            nsx.rx_ipv4_tcp_verify_dev(arena, offs, mask=mask, ip_raw=ipr, tcp_raw=tcpr, tune=tune)
            got = (host(mask).view(np.uint64), u16(ipr), u16(tcpr))
        else:
            nsx.rx_ipv6_tcp_verify_dev(arena, offs, mask=mask, tcp_raw=tcpr, tune=tune)
            got = (host(mask).view(np.uint64), u16(tcpr))
        for w, g, what in zip(want, got, names):
            if what == "mask":
                assert r.n % 64 == 0 or int(g[-1]) >> (r.n % 64) == 0, ("bits past n", tune)
                w, g = _gro.valid_bits(w, r.n), _gro.valid_bits(g, r.n)
            bad = np.nonzero(w != g)[0]
            assert bad.size == 0, (what, tune, f"span {r.span}", bad[:8], g[bad[:8]], w[bad[:8]])
    _check_arena(arena, r.pieces(), "rx")


# ------------------------------------------------------------------ the ragged checksum and verify
@mixes
@placements
def test_far_csum_and_verify_ragged(arena, placement, mix):
    """nsx_csum_ragged_dev / nsx_verify_ragged_dev: the span is in contract here (no segment limit), so its own sum is
    checked — 16-bit markers at even and odd addresses around its byte 2^31, on both sides of absolute byte 2^32 and
    in its last row must all be counted, once, with the right byte order. With and without prefix partials; the
    partials make every third segment, and the span, verify."""
    r = _far.csum_batch(placement, mix)
    _put(arena, r.pieces())
    offs = _offs(r)
    plain = O.c_batch(r.buf, r.n, offsets=r.offs)
    rng = np.random.default_rng(7)
    part = rng.integers(0, 1 << 31, r.n, dtype=np.uint64).astype(np.uint32)
    fix = np.arange(r.n) % 3 == 0
    fix[r.span] = True
    part[fix] = 0xFFFF - plain[fix].astype(np.uint32)
    for p in (None, part):
        want = plain if p is None else O.c_batch(r.buf, r.n, offsets=r.offs, partial=p)
        dp = None if p is None else _d(p)
        out = torch.full((r.n,), 0x5A5A, dtype=torch.int16, device="cuda")
        raw = torch.full((r.n,), 0x5A5A, dtype=torch.int16, device="cuda")
        nsx.ragged_dev(arena, offs, partial=dp, out=out)
        ok = nsx.verify_ragged_dev(arena, offs, partial=dp, raw=raw)
        for g, what in ((u16(out), "csum"), (u16(raw), "verify raw")):
            bad = np.nonzero(g != want)[0]
            assert bad.size == 0, (what, p is not None, f"span {r.span}", bad[:8], g[bad[:8]], want[bad[:8]])
        assert np.array_equal(host(ok) != 0, want == 0xFFFF), ("ok", p is not None)
        if p is not None:
            assert want[r.span] == 0xFFFF and (want[fix] == 0xFFFF).all()
    _check_arena(arena, r.pieces(), "ragged")


# ------------------------------------------------------------------ the parse pass
@mixes
@placements
def test_far_tcp_parse(arena, placement, mix):
    """nsx_tcp_parse_dev: every field and status; data_off is an absolute offset, so behind the span it is the twin's
    value plus D (above 2^32). The span parses as its head says — its length is 64-bit, not its low word."""
    r = _far.parse_batch(placement, mix)
    want = _far.parse_model(r)
    _put(arena, r.pieces())
    got = nsx.tcp_parse_dev(arena, _offs(r))
    for k, dt in nsx.PARSE_FIELDS:
        g = host(got[k]).view(_U[dt])
        bad = np.nonzero(g != want[k])[0]
        assert bad.size == 0, (k, f"span {r.span}", bad[:8], g[bad[:8]], want[k][bad[:8]])
    assert (want["data_off"][r.span + 1:].max() >= _far.TWO32) and want["status"][r.span] == nsx.PARSE_OK
    _check_arena(arena, r.pieces(), "parse")


# ------------------------------------------------------------------ receive coalescing
@mixes
@placements
@pytest.mark.parametrize("flow", [False, True], ids=["gro", "gro_flow"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_far_gro(arena, gro_data, ipver, flow, placement, mix):
    """nsx_gro_* and nsx_gro_flow_*: every output array, n_super and d_order. The span's valid bit is set and it is no
    member; in wrap_frame its head is the in-order frame between the last near and the first far frame, and the two
    runs are not joined through it; in the straddle placements the run across byte 2^32 is merged and its payload is
    compared byte for byte (the whole data array is). The data array is given at its worst-case extent and nothing
    past the packed payloads is written."""
    r, valid = _far.gro_batch(ipver, placement, mix, flow)
    nb = r.buf.size
    w, o = _gro_gpu.want(r.buf, r.offs, valid, ipver, flow)
    assert o["frame_seg"][r.span] == 0xFFFFFFFF
    if placement[0] == "straddle":
        assert o["frame_cnt"][o["frame_seg"][_far.crossing(r.far_offs)[0]]] == _far.BRIDGE_FAR
    _put(arena, r.pieces())
    out = _gro_gpu.filled(r.n, ipver, 1, flow)
    order = out.pop("order", None)
    assert nb <= 8 << 20
    gro_data[:8 << 20] = _gro_gpu.FILL  # what an earlier case's payloads may have left
    out["data"] = gro_data
    kw = dict(order=order) if flow else {}
    res = _gro_gpu.fn(ipver, flow)(arena, _offs(r), _gro_gpu.d_valid(valid, r.n), out=out, **kw)
    got = {k: host(res[k][:nb] if k == "data" else res[k]).view(_gro_gpu._NP[dt])
           for k, (dt, _) in _gro_gpu.sizes(r.n, ipver, nb, flow).items()}
    _gro_gpu.same(got, w, f"{_far.pid(placement)} {mix}")
    assert _all_equal(gro_data[nb:], _gro_gpu.FILL), "data bytes written past the twin's extent"
    _check_arena(arena, r.pieces(), "gro")


# ------------------------------------------------------------------ the NAT rewrite
@mixes
@placements
@pytest.mark.parametrize("ipver", [4, 6])
def test_far_nat_rewrite_in_place(arena, ipver, placement, mix):
    """nsx_nat_ipv4_tcp_rewrite_dev / nsx_nat_ipv6_tcp_rewrite_dev write in place: the hit mask and the arena. The
    span's head is a frame whose tuple has a rule and whose valid bit is set, and stays as it is; far frames are
    rewritten at their addresses above 2^32; nothing else in 4 GiB changes."""
    r, valid, table, slots, dec = _far.nat_batch(ipver, placement, mix)
    new, hit = _far.nat_model(ipver, r.buf, r.offs, valid, table, slots, dec)
    assert not hit[r.span] and hit[r.span + 1:].sum() > 100
    _put(arena, r.pieces())
    d_hit = torch.full(((r.n + 63) // 64,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    fn = nsx.nat_ipv4_tcp_rewrite_dev if ipver == 4 else nsx.nat_ipv6_tcp_rewrite_dev
    fn(arena, _offs(r), _gro_gpu.d_valid(valid, r.n), dev(table), slots, ttl_dec=dec, hit=d_hit)
    g = _gro.valid_bits(host(d_hit).view(np.uint64), r.n)
    bad = np.nonzero(g != hit)[0]
    assert bad.size == 0, (f"span {r.span}", bad[:8], g[bad[:8]], hit[bad[:8]])
    assert np.array_equal(host(d_hit).view(np.uint64), mask_words(hit.astype(np.uint8)))
    _check_arena(arena, r.pieces(new), "nat")


# ------------------------------------------------------------------ the build passes: the arena is d_out
def _slot_lens(rng, flen):
    """Each frame's slot: its length rounded up to 4, every fifth with a gap of 4-64 bytes behind it."""
    s = (np.asarray(flen, np.uint64) + np.uint64(3)) & ~np.uint64(3)
    s[::5] += (rng.integers(1, 17, s[::5].size) * 4).astype(np.uint64)
    return s


def _out_pieces(start, twin, want, n_near):
    """The expected twin output buffer as device pieces: everything below the twin's first far slot (the near slots
    and the untouched bytes behind them) at its own address, the far slots BUILD_D higher."""
    far_t = int(twin[n_near])
    return [(0, want[:far_t]), (int(start[n_near]), want[far_t:])]


def _case(rng, ipver, n, mix):
    lens = rng.integers(0, (81 if mix == "small" else 1401), n)
    ob = [_tx.opt_bytes(rng, sorted(_tx.OPT_SETS)[i % len(_tx.OPT_SETS)]) if i % 3 == 1 else b"" for i in range(n)]
    return _tx.Case(rng, ipver, lens, opts=ob, lead=int(rng.integers(4)))


def _tx_inputs(c):
    return dict(ip={k: _d(v.reshape(-1)) for k, v in c.ip.items()}, fields={k: _d(v) for k, v in c.fields.items()},
                data=_d(c.data), data_off=_d(c.data_off), opts=_d(c.opts), opt_off=_d(c.opt_off))


def _raw_same(raw, wraw, what):
    bad = np.nonzero(raw != wraw)[0]
    assert bad.size == 0, (what, bad[:8], raw[bad[:8]], wraw[bad[:8]])


@mixes
def test_far_tcp_build_slots(arena, mix):
    """nsx_tcp_build_dev with d_out_off up to and past 2^32: 200 images near 0, 400 from 2^32 - 700 upward, one across
    byte 2^32; each over its own pseudo-header partial."""
    rng = np.random.default_rng([0xFB0, _far.MIXES.index(mix)])
    n = _far.BUILD_NEAR + _far.BUILD_FAR
    c = _case(rng, 4, n, mix)
    start, twin = _far.build_slots(_slot_lens(rng, c.wire))
    ps = _tx.pseudo_headers(c)
    pw = ps.reshape(n, 6, 2).astype(np.uint32)
    part = ((pw[..., 0] << 8) | pw[..., 1]).sum(1).astype(np.uint32)
    want, wraw = O.c_go_tcp_build_mt(c.fields, c.data, c.data_off, twin, ps, opts=c.opts, opt_off=c.opt_off)
    arena.zero_()
    inp = _tx_inputs(c)
    raw = torch.full((n,), 0x5A5A, dtype=torch.int16, device="cuda")
    nsx.tcp_build_dev(inp["fields"], inp["data"], inp["data_off"], arena, _d(start), opts=inp["opts"],
                      opt_off=inp["opt_off"], partial=_d(part), raw=raw)
    _raw_same(u16(raw), wraw, "tcp build raw")
    _check_arena(arena, _out_pieces(start, twin, want, _far.BUILD_NEAR), "tcp build")


@mixes
@pytest.mark.parametrize("ipver", [4, 6])
def test_far_tx_slots(arena, ipver, mix):
    """nsx_tx_ipv4_tcp_build_dev / nsx_tx_ipv6_tcp_build_dev with the same far slots: whole datagrams."""
    rng = np.random.default_rng([0xFB1, ipver, _far.MIXES.index(mix)])
    n = _far.BUILD_NEAR + _far.BUILD_FAR
    c = _case(rng, ipver, n, mix)
    start, twin = _far.build_slots(_slot_lens(rng, c.flen))
    want, wraw = _tx.expected(c, twin, fill=0)
    arena.zero_()
    inp = _tx_inputs(c)
    raw = torch.full((n,), 0x5A5A, dtype=torch.int16, device="cuda")
    fn = nsx.tx_ipv4_tcp_build_dev if ipver == 4 else nsx.tx_ipv6_tcp_build_dev
    fn(inp["ip"], inp["fields"], inp["data"], inp["data_off"], arena, _d(start), opts=inp["opts"],
       opt_off=inp["opt_off"], raw=raw)
    _raw_same(u16(raw), wraw, "tx raw")
    _check_arena(arena, _out_pieces(start, twin, want, _far.BUILD_NEAR), "tx")


@mixes
@pytest.mark.parametrize("ipver", [4, 6])
def test_far_tso_slots(arena, ipver, mix):
    """nsx_tso_ipv4_tcp_build_dev / nsx_tso_ipv6_tcp_build_dev: the frames of 60 super-segments, the first third of
    them near 0 and the others from 2^32 - 700 upward — the cut falls inside a super-segment."""
    rng = np.random.default_rng([0xFB2, ipver, _far.MIXES.index(mix)])
    mss = 64 if mix == "small" else 1400
    lens = rng.integers(0, 20 * mss, 60)
    ob = [_tx.opt_bytes(rng, ("mss", "nop_nop_k2len10", "k2len40")[i % 3]) if i % 3 == 1 else b"" for i in range(60)]
    b = _tso.Batch(rng, ipver, lens, mss, opts=ob, lead=int(rng.integers(4)))
    c = _tso.expand(b)
    n_near = next(f for f in range(b.nf // 3, b.nf) if b.seg[f - 1] == b.seg[f])  # the cut inside a super-segment
    start, twin = _far.build_slots(_slot_lens(rng, c.flen), n_near)
    want, wraw, _ = _tso.expected(b, off=twin, fill=0)
    arena.zero_()
    s = b.sup
    raw = torch.full((b.nf,), 0x5A5A, dtype=torch.int16, device="cuda")
    fn = nsx.tso_ipv4_tcp_build_dev if ipver == 4 else nsx.tso_ipv6_tcp_build_dev
    fn({k: _d(v.reshape(-1)) for k, v in s.ip.items()}, {k: _d(v) for k, v in s.fields.items()}, _d(s.data),
       _d(s.data_off), _d(b.mss), _d(b.first), _d(b.seg), arena, _d(start), opts=_d(s.opts), opt_off=_d(s.opt_off),
       raw=raw)
    _raw_same(u16(raw), wraw, "tso raw")
    _check_arena(arena, _out_pieces(start, twin, want, n_near), "tso")


GIANT = _far.TWO32 + 100
DATA_AT = 1 << 20  # the payloads' place in the arena: behind the near slots, and its far part behind the far slots


@pytest.mark.parametrize("ipver", [4, 6])
def test_far_tx_payload_of_2_32_plus_100_is_not_built_and_later_payloads_come_from_above_it(arena, ipver):
    """The transmit pass's contract: a frame whose length does not fit its 16-bit length field "is not built: nothing
    is written for it, padding included, and d_tcp_raw[i] = 0". Segment 100's payload is 2^32 + 100 bytes — read by
    its low word it would be a 100-byte frame. d_data is the arena itself (a second view of d_out), so the segments
    behind it take their payloads from d_data_off >= 2^32 and must build correctly, into the far slots as well."""
    rng = np.random.default_rng([0xFB3, ipver])
    n, g = _far.BUILD_NEAR + _far.BUILD_FAR, 100
    lens = rng.integers(0, 401, n)
    lens[g] = 0  # in the twin; GIANT on the device
    ob = [_tx.opt_bytes(rng, sorted(_tx.OPT_SETS)[i % len(_tx.OPT_SETS)]) if i % 3 == 1 else b"" for i in range(n)]
    c = _tx.Case(rng, ipver, lens, opts=ob, lead=int(rng.integers(4)))
    start, twin = _far.build_slots(_slot_lens(rng, c.flen))
    want, wraw = _tx.expected(c, twin, fill=0)
    want[int(twin[g]):int(twin[g + 1])] = 0  # nothing is written for it
    wraw[g] = 0
    cut = int(c.data_off[g])
    data_off = c.data_off + np.uint64(DATA_AT)
    data_off[g + 1:] += np.uint64(GIANT)
    assert int(data_off[g + 1] - data_off[g]) == GIANT and int(data_off[-1]) + 8 <= _far.ARENA
    payloads = [(DATA_AT, c.data[:cut]), (DATA_AT + cut + GIANT, c.data[cut:])]
    out = _out_pieces(start, twin, want, _far.BUILD_NEAR)
    assert out[0][0] + len(out[0][1]) + _far.GUARD <= DATA_AT - _far.GUARD  # the near slots end below the payloads
    assert out[1][0] + len(out[1][1]) + _far.GUARD <= payloads[1][0] - _far.GUARD  # and the far slots too
    _put(arena, payloads)
    raw = torch.full((n,), 0x5A5A, dtype=torch.int16, device="cuda")
    fn = nsx.tx_ipv4_tcp_build_dev if ipver == 4 else nsx.tx_ipv6_tcp_build_dev
    fn({k: _d(v.reshape(-1)) for k, v in c.ip.items()}, {k: _d(v) for k, v in c.fields.items()}, arena, _d(data_off),
       arena, _d(start), opts=_d(c.opts), opt_off=_d(c.opt_off), raw=raw)
    got = u16(raw)
    assert got[g] == 0, f"the 2^32 + 100 byte payload was built: raw {got[g]:#x}"
    _raw_same(got, wraw, "tx raw")
    _check_arena(arena, out + payloads, "tx with a 2^32 + 100 byte payload")
