"""Segmentation offload on the GPU (nsx_tso_ipv4_tcp_build_* / nsx_tso_ipv6_tcp_build_*): every output byte, raw sum
and padding byte against the expected frames of tests/_tso.py (the super-segment batch expanded on the CPU, then the
Go-faithful sender loop of tests/_tx.py; held to the oracle frames by tests/test_tso_abi.py). Bit-exact throughout."""
import functools

import numpy as np
import pytest

import _tso
import _tx
from _gpu import dev, host, setup_gpu, torch, u16, nsx

pytestmark = pytest.mark.gpu

_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
           np.dtype(np.uint64): np.int64}
FILL = 0xAB


def setup_module(module):
    setup_gpu()


def _d(a):
    a = np.ascontiguousarray(a)
    return dev(a.view(_SIGNED[a.dtype]))


def _inputs(b, null=()):
    """The batch's arrays in HBM; null: the optional members passed as NULL."""
    s = b.sup
    return dict(ip={k: _d(v.reshape(-1)) for k, v in s.ip.items() if k not in null},
                fields={k: _d(v) for k, v in s.fields.items() if k not in null},
                data=_d(s.data), data_off=_d(s.data_off), mss=_d(b.mss), first=_d(b.first), seg=_d(b.seg),
                opts=None if s.opts is None else _d(s.opts), opt_off=None if s.opt_off is None else _d(s.opt_off))


def _fn(ipver):
    return nsx.tso_ipv4_tcp_build_dev if ipver == 4 else nsx.tso_ipv6_tcp_build_dev


def _run(b, off=None, tune=None, want_raw=True, inp=None, stream=None):
    """One device call over a FILL-filled buffer of off[n_frames] bytes: (buffer, raw sums or None)."""
    inp = _inputs(b) if inp is None else inp
    off = b.off if off is None else off
    out = torch.full((int(off[-1]),), FILL, dtype=torch.uint8, device="cuda")
    raw = torch.full((b.nf,), 0x5A5A, dtype=torch.int16, device="cuda") if want_raw else None
    _fn(b.ipver)(inp["ip"], inp["fields"], inp["data"], inp["data_off"], inp["mss"], inp["first"], inp["seg"], out,
                 _d(off), opts=inp["opts"], opt_off=inp["opt_off"], raw=raw, stream=stream, tune=tune)
    return host(out), (u16(raw) if want_raw else None)


def _same(b, c, off, got, raw, want, wraw):
    if raw is not None:
        bad = np.nonzero(raw != wraw)[0]
        assert bad.size == 0, (bad[:8], b.seg[bad[:8]], raw[bad[:8]], wraw[bad[:8]])
    if not np.array_equal(got, want):
        d = np.nonzero(got != want)[0]
        f = int(np.searchsorted(np.asarray(off, np.uint64), d[0], side="right")) - 1
        s = int(b.seg[f])
        raise AssertionError(f"{d.size} bytes differ, first at {d[0]}: frame {f} (super-segment {s}, frame "
                             f"{f - int(b.first[s])} of it), byte {d[0] - int(off[f])} of {int(c.flen[f])}: "
                             f"got {got[d[:8]]}, want {want[d[:8]]}")


def _opt_list(rng, n, every=3, keys=None):
    keys = sorted(_tx.OPT_SETS) if keys is None else keys
    return [_tx.opt_bytes(rng, keys[i % len(keys)]) if i % every else b"" for i in range(n)]


def _cut_lengths(mss):
    return sorted({0, 1, mss - 1, mss, mss + 1, 3 * mss - 1, 3 * mss, 3 * mss + 1})


# ---------------------------------------------------------------- cut points
@functools.lru_cache(maxsize=None)
def _cut_case(ipver, mss, opts):
    """Every cut length of one mss, three times over in mixed order behind one lead byte (so the slices' source
    alignment takes 0-3), with the option sets of tests/_tx.py — `nop` and `k2len41` (unaligned headers) among them."""
    rng = np.random.default_rng(0x200 + 16 * mss + 2 * ipver + opts)
    lens = np.array(_cut_lengths(mss) * 3)
    rng.shuffle(lens)
    ob = _opt_list(rng, lens.size, every=3) if opts else None
    if opts:
        assert {len(_tx.opt_bytes(rng, "nop")), len(_tx.opt_bytes(rng, "k2len41"))} <= {len(x) for x in ob}
    b = _tso.Batch(rng, ipver, lens, mss, opts=ob, lead=1)
    want, wraw, c = _tso.expected(b, fill=FILL)
    return b, c, want, wraw, _inputs(b)


@pytest.mark.parametrize("run_segs", [1, 16, 64])
@pytest.mark.parametrize("kernel", [0, nsx.KERNEL_BUILD_PLAIN, nsx.KERNEL_BUILD_GENERAL],
                         ids=["auto", "plain", "general"])
@pytest.mark.parametrize("opts", [False, True], ids=["noopt", "opts"])
@pytest.mark.parametrize("mss", [1460, 1448, 1461, 537, 8960, 3])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_cut_points(ipver, mss, opts, kernel, run_segs):
    """4-aligned (1460, 1448, 8960) and unaligned (1461, 537, 3) slices; one-, two- and many-row frames."""
    b, c, want, wraw, inp = _cut_case(ipver, mss, opts)
    got, raw = _run(b, tune=dict(kernel=kernel, run_segs=run_segs), inp=inp)
    _same(b, c, b.off, got, raw, want, wraw)


# ---------------------------------------------------------------- groups that straddle super-segments
@functools.lru_cache(maxsize=None)
def _straddle_case(ipver, opts=True):
    """112 super-segments of 1, 15, 16, 17, 45 and 130 frames: 16 shuffled rounds of the six (224 frames, 14 groups
    of 16) with a single-frame super-segment after each, so that round r starts at lane r of a 16-frame group and
    super-segment boundaries fall on every lane position; mss 3, 537, 1448 and 1460 mixed within the groups; 3,600
    frames."""
    rng = np.random.default_rng(0x2A0 + ipver)
    cnt = np.concatenate([np.append(rng.permutation([1, 15, 16, 17, 45, 130]), 1) for _ in range(16)])
    assert set((np.cumsum(cnt) % 16).tolist()) == set(range(16))
    mss = np.array([(1460, 3, 537, 1448)[i % 4] for i in range(cnt.size)], np.uint32)
    lens = cnt * mss - rng.integers(0, np.minimum(mss, 5))  # the last frame short by 0-4 bytes
    ob = _opt_list(rng, cnt.size, every=3) if opts else None
    b = _tso.Batch(rng, ipver, lens, mss, opts=ob, lead=2)
    assert np.array_equal(np.diff(b.first), cnt) and int(b.sup.data_off[-1]) < 4 << 20
    want, wraw, c = _tso.expected(b, fill=FILL)
    return b, c, want, wraw, _inputs(b)


@pytest.mark.parametrize("tune", [None, dict(run_segs=16), dict(run_segs=64), dict(run_segs=16, kernel=2),
                                  dict(run_segs=5, kernel=3)], ids=["default", "g16", "g64", "g16plain", "g5general"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_groups_straddle_super_segments(ipver, tune):
    b, c, want, wraw, inp = _straddle_case(ipver)
    got, raw = _run(b, tune=tune, inp=inp)
    _same(b, c, b.off, got, raw, want, wraw)


# ---------------------------------------------------------------- the field rules
def _rules_batch(ipver):
    rng = np.random.default_rng(0x2B0 + ipver)
    n = 36
    mss = np.array([(1460, 536, 7, 2000)[i % 4] for i in range(n)], np.uint32)
    lens = np.array([int(rng.integers(0, 6 * m)) for m in mss])
    lens[:4] = [5 * 1460, 3 * 536 + 1, 7 * 40, 2000]
    b = _tso.Batch(rng, ipver, lens, mss, opts=_opt_list(rng, n), lead=3)
    s = b.sup
    s.fields["control"][:] = np.resize(np.array([0xFF, 0x19, 0x89, 0x18, 0x11, 0x90, 0x80, 0x02, 0x10], np.uint8), n)
    s.fields["seq_num"][:] = (0x100000000 - rng.integers(0, 2 * mss)).astype(np.uint32)  # within 2·mss of 2^32
    s.fields["seq_num"][0] = 0xFFFFFFFF
    s.ip["ident"][:] = 0xFFFE
    return b


@pytest.mark.parametrize("null", [(), ("ident",), ("offset",), ("ttl", "tclass", "flow"),
                                  ("ident", "offset", "ttl", "tclass", "flow")],
                         ids=["all", "noident", "nooffset", "nottl", "allnull"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_field_rules(ipver, null):
    """control 0xFF (FIN / PSH on the last frame only, CWR on the first only, the other five bits on every frame),
    sequence numbers that wrap inside their super-segment, ident 0xFFFE wrapping to 0, and NULL ident (0 + j), NULL
    offset (computeOffset()), NULL ttl / tclass / flow (64 / 0 / 0)."""
    b = _rules_batch(ipver)
    want, wraw, c = _tso.expected(b, fill=FILL, null=null)
    ctl = c.fields["control"][b.seg == 0]
    assert ctl.size == 5 and ctl.tolist() == [0xF6, 0x76, 0x76, 0x76, 0x7F]
    assert c.fields["seq_num"][:3].tolist() == [0xFFFFFFFF, 1459, 2919]
    assert (c.ip["ident"][:5].tolist() == [0, 1, 2, 3, 4]) if "ident" in null else \
        (c.ip["ident"][:5].tolist() == [0xFFFE, 0xFFFF, 0, 1, 2])
    for tune in (None, dict(run_segs=16)):
        got, raw = _run(b, tune=tune, inp=_inputs(b, null=null))
        _same(b, c, b.off, got, raw, want, wraw)


# ---------------------------------------------------------------- no cut: the transmit pass itself
@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_without_a_cut_equals_the_transmit_pass(ipver):
    """Every len_s <= mss[s]: one frame per super-segment, and the output and raw sums equal
    nsx_tx_ipv4_tcp_build_dev / nsx_tx_ipv6_tcp_build_dev on the same inputs, byte for byte."""
    rng = np.random.default_rng(0x2C0 + ipver)
    n = 300
    mss = rng.integers(1, 3000, n).astype(np.uint32)
    lens = rng.integers(0, mss + 1)
    lens[:3] = [0, int(mss[1]), 1]
    b = _tso.Batch(rng, ipver, lens, mss, opts=_opt_list(rng, n), lead=1)
    assert b.nf == n and np.array_equal(b.off, b.sup.packed())
    inp = _inputs(b)
    got, raw = _run(b, inp=inp)
    plain = torch.full((int(b.off[-1]),), FILL, dtype=torch.uint8, device="cuda")
    praw = torch.zeros(n, dtype=torch.int16, device="cuda")
    tx = nsx.tx_ipv4_tcp_build_dev if ipver == 4 else nsx.tx_ipv6_tcp_build_dev
    tx(inp["ip"], inp["fields"], inp["data"], inp["data_off"], plain, _d(b.off), opts=inp["opts"],
       opt_off=inp["opt_off"], raw=praw)
    assert np.array_equal(got, host(plain)) and np.array_equal(raw, u16(praw))
    want, wraw, c = _tso.expected(b, fill=FILL)
    _same(b, c, b.off, got, raw, want, wraw)


# ---------------------------------------------------------------- over-long frames
@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_over_long_frames_are_not_built(ipver):
    """mss 65535: a full frame's TCP part (65555 B) does not fit the IP length field — those slots keep their
    sentinel bytes and get raw sum 0; the super-segment's short last frame and the neighbours are built."""
    rng = np.random.default_rng(0x2D0 + ipver)
    lens = [700, 2 * 65535 + 100, 0, 65535, 1460 * 3, 65000]
    mss = np.array([1460, 65535, 65535, 65535, 1460, 65535], np.uint32)
    b = _tso.Batch(rng, ipver, lens, mss)
    want, wraw, c = _tso.expected(b, fill=FILL)
    over = np.nonzero(c.wire > _tx.WIRE_MAX[ipver])[0]
    assert over.tolist() == [1, 2, 5] and (wraw[over] == 0).all() and (np.delete(wraw, over) != 0).all()
    for f in over:
        assert (want[int(b.off[f]):int(b.off[f + 1])] == FILL).all()
    for tune in (None, dict(run_segs=16)):
        got, raw = _run(b, tune=tune)
        _same(b, c, b.off, got, raw, want, wraw)


# ---------------------------------------------------------------- layout
@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_gaps_and_sentinels(ipver):
    """Frame slots longer than frame + padding, from a nonzero first offset: only [frame, round_up4(frame)) of each
    slot is written."""
    b, c, _, _, inp = _straddle_case(ipver)
    rng = np.random.default_rng(0x2E0 + ipver)
    gap = 4 * rng.integers(0, 9, b.nf).astype(np.uint64) * (rng.random(b.nf) < 0.5)
    off = np.zeros(b.nf + 1, np.uint64)
    off[1:] = np.cumsum(np.diff(b.off) + gap)
    off += np.uint64(52)
    want, wraw, _ = _tso.expected(b, off, fill=FILL)
    assert (want[:52] == FILL).all() and (want == FILL).sum() > gap.sum() // 2
    for tune in (None, dict(run_segs=16, kernel=nsx.KERNEL_BUILD_PLAIN)):
        got, raw = _run(b, off, tune=tune, inp=inp)
        _same(b, c, off, got, raw, want, wraw)


@pytest.mark.parametrize("counts", [(1,), (2,), (5, 12), (1, 45, 19)], ids=["f1", "f2", "f17", "f65"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_group_tails(ipver, counts):
    """Batches of 1, 2, 17 and 65 frames: the last group is short, and frame_seg / frame_first end with it."""
    rng = np.random.default_rng(0x2F0 + ipver + sum(counts))
    cnt = np.array(counts)
    mss = np.array([(537, 1460, 8)[i % 3] for i in range(cnt.size)], np.uint32)
    b = _tso.Batch(rng, ipver, cnt * mss - 1, mss, opts=_opt_list(rng, cnt.size, every=2), lead=1)
    assert b.nf == sum(counts)
    want, wraw, c = _tso.expected(b, fill=FILL)
    for tune in (None, dict(run_segs=16), dict(run_segs=64)):
        got, raw = _run(b, tune=tune)
        _same(b, c, b.off, got, raw, want, wraw)


@pytest.mark.parametrize("lead", [1, 2, 3])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_payload_source_alignment(ipver, lead):
    """The payload array starting 1-3 bytes off a dword, with 4-multiple mss: every slice of the batch shares that
    misalignment (the general composition), on every path."""
    rng = np.random.default_rng(0x300 + ipver + lead)
    n = 24
    mss = np.array([(1460, 1448, 536, 8960)[i % 4] for i in range(n)], np.uint32)
    lens = 4 * rng.integers(0, mss)
    b = _tso.Batch(rng, ipver, lens, mss, opts=_opt_list(rng, n, keys=["mss", "k2len40", "nop"]), lead=lead)
    want, wraw, c = _tso.expected(b, fill=FILL)
    assert (c.data_off[:-1] % 4 == lead).all()
    for tune in (None, dict(run_segs=16, kernel=nsx.KERNEL_BUILD_PLAIN), dict(kernel=nsx.KERNEL_BUILD_GENERAL)):
        got, raw = _run(b, tune=tune)
        _same(b, c, b.off, got, raw, want, wraw)


# ---------------------------------------------------------------- closing the loop on the device
@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_frames_pass_the_receive_and_parse_kernels(ipver):
    """4-multiple frame lengths in the packed layout: the build's d_out / d_out_off go straight into the fused
    receive pass, which finds every frame valid, and nsx_tcp_parse_dev reads back each frame's own sequence number
    and control byte."""
    rng = np.random.default_rng(0x310 + ipver)
    n = 60
    mss = np.array([(1460, 1448, 536, 8)[i % 4] for i in range(n)], np.uint32)
    lens = 4 * rng.integers(0, 2 * mss)
    # options the reference's parse loop walks (tcp.go:160-179): MSS, and NOPs ended by the zero padding
    b = _tso.Batch(rng, ipver, lens, mss, opts=_opt_list(rng, n, keys=["mss", "nop_nop"]))
    b.sup.fields["control"][:] = np.resize(np.array([0xFF, 0x19, 0x89, 0x18], np.uint8), n)
    c = _tso.expand(b)
    assert not (c.flen % 4).any() and b.nf > 2 * n
    inp = _inputs(b)
    d_off = _d(b.off)
    d_out = torch.full((int(b.off[-1]),), FILL, dtype=torch.uint8, device="cuda")
    _fn(ipver)(inp["ip"], inp["fields"], inp["data"], inp["data_off"], inp["mss"], inp["first"], inp["seg"], d_out,
               d_off, opts=inp["opts"], opt_off=inp["opt_off"])
    tcp_raw = torch.empty(b.nf, dtype=torch.int16, device="cuda")
    if ipver == 4:
        ip_raw = torch.empty(b.nf, dtype=torch.int16, device="cuda")
        mask = nsx.rx_ipv4_tcp_verify_dev(d_out, d_off, ip_raw=ip_raw, tcp_raw=tcp_raw)
        assert (u16(ip_raw) == 0xFFFF).all()
    else:
        mask = nsx.rx_ipv6_tcp_verify_dev(d_out, d_off, tcp_raw=tcp_raw)
    ones = np.packbits(np.ones(b.nf, np.uint8), bitorder="little")
    ones = np.concatenate([ones, np.zeros(-ones.size % 8, np.uint8)]).view(np.uint64)
    assert np.array_equal(host(mask).view(np.uint64), ones) and (u16(tcp_raw) == 0xFFFF).all()
    # the TCP parts: segment f = the frame's TCP image and, as trailing payload, the next frame's IP header
    iph = _tx.IPH[ipver]
    seg_off = b.off.copy()
    seg_off[-1] -= np.uint64(iph)
    got = nsx.tcp_parse_dev(d_out[iph:], _d(seg_off), want=["seq_num", "control", "status"])
    assert not host(got["status"]).any()
    assert np.array_equal(host(got["seq_num"]).view(np.uint32), c.fields["seq_num"])
    assert np.array_equal(host(got["control"]), c.fields["control"])


# ---------------------------------------------------------------- host calls
@pytest.mark.parametrize("chunk", [0, 64 << 10], ids=["onechunk", "chunks64k"])
@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("mem", ["pageable", "pinned"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_host_calls(ipver, mem, shards, chunk):
    """nsx_tso_ipv4_tcp_build_host / nsx_tso_ipv6_tcp_build_host from and to pageable or pinned memory, 1 or 3 shards
    on the device, in one chunk or in 64 KiB chunks (the 130-frame super-segments exceed that and go alone): frames
    and raw sums equal tests/_tso.py."""
    b, c, want, wraw, _ = _straddle_case(ipver)
    s = b.sup
    fn = nsx.tso_ipv4_tcp_build_host if ipver == 4 else nsx.tso_ipv6_tcp_build_host
    kw = dict(frame_first=b.first, frame_seg=b.seg, out_off=b.off, opts=s.opts, opt_off=s.opt_off,
              tune=dict(shards_per_device=shards, chunk_bytes=chunk))
    if mem == "pinned":
        dp, op = nsx.PinnedBuffer(s.data.nbytes), nsx.PinnedBuffer(int(b.off[-1]))
        dp.array[:] = s.data
        op.array[:] = FILL
        got, raw = fn(s.ip, s.fields, dp.array, s.data_off, b.mss, out=op.array, **kw)
        got = got.copy()
        dp.free()
        op.free()
    else:
        got, raw = fn(s.ip, s.fields, s.data, s.data_off, b.mss, out=np.full(int(b.off[-1]), FILL, np.uint8), **kw)
    _same(b, c, b.off, got, raw, want, wraw)


@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_host_call_defaults_and_gaps(ipver):
    """The frame map left to the binding (nsx_tso_count_host / nsx_tso_layout_host), no raw sums, NULL optional
    fields; then slots with gaps over a sentinel buffer in small chunks: the caller's bytes between frames stay."""
    b = _rules_batch(ipver)
    s = b.sup
    fn = nsx.tso_ipv4_tcp_build_host if ipver == 4 else nsx.tso_ipv6_tcp_build_host
    null = ("ident", "offset", "ttl", "tclass", "flow")
    want, wraw, c = _tso.expected(b, null=null)
    got, raw = fn({k: v for k, v in s.ip.items() if k not in null}, {k: v for k, v in s.fields.items() if k not in null},
                  s.data, s.data_off, b.mss, opts=s.opts, opt_off=s.opt_off, want_raw=False)
    assert raw is None
    _same(b, c, b.off, got, None, want, wraw)
    off = b.off + np.uint64(8) * np.arange(b.nf + 1, dtype=np.uint64) + np.uint64(12)
    want, wraw, c = _tso.expected(b, off, fill=FILL)
    got, raw = fn(s.ip, s.fields, s.data, s.data_off, b.mss, out_off=off, opts=s.opts, opt_off=s.opt_off,
                  out=np.full(int(off[-1]), FILL, np.uint8), tune=dict(chunk_bytes=8192))
    _same(b, c, off, got, raw, want, wraw)


# ---------------------------------------------------------------- graph capture
@pytest.mark.parametrize("ipver", [4, 6])
def test_tso_device_call_captures_into_a_graph(ipver):
    """The device call allocates nothing and never synchronises: captured with torch.cuda.graph on a side stream and
    replayed once, it builds the exact frames."""
    b, c, want, wraw, inp = _straddle_case(ipver)
    d_off = _d(b.off)
    out = torch.full((int(b.off[-1]),), FILL, dtype=torch.uint8, device="cuda")
    raw = torch.zeros(b.nf, dtype=torch.int16, device="cuda")
    fn = _fn(ipver)
    args = (inp["ip"], inp["fields"], inp["data"], inp["data_off"], inp["mss"], inp["first"], inp["seg"])
    # a first call outside capture (library and device-info setup), into a buffer of its own
    fn(*args, torch.empty_like(out), d_off, opts=inp["opts"], opt_off=inp["opt_off"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn(*args, out, d_off, opts=inp["opts"], opt_off=inp["opt_off"], raw=raw)
    torch.cuda.synchronize()
    assert (host(out) == FILL).all()  # capture ran nothing
    g.replay()
    _same(b, c, b.off, host(out), u16(raw), want, wraw)
