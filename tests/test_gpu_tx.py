"""The fused transmit pass on the GPU (nsx_tx_ipv4_tcp_build_* / nsx_tx_ipv6_tcp_build_*): every output byte, raw
sum and padding byte against the expected frames of tests/_tx.py (the Go-faithful sender loop + numpy IP headers,
held to O.ipv4_tcp_frame / O.ipv6_tcp_frame by tests/test_tx_abi.py). Bit-exact throughout."""
import functools

import numpy as np
import pytest

import _tx
from _gpu import dev, host, setup_gpu, torch, u16, nsx

pytestmark = pytest.mark.gpu

_OPT_SETS = _tx.OPT_SETS  # tests/test_gpu_parity.py's option sets, restated in tests/_tx.py
_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
           np.dtype(np.uint64): np.int64}


def setup_module(module):
    setup_gpu()


def _d(a):
    a = np.ascontiguousarray(a)
    return dev(a.view(_SIGNED[a.dtype]))


def _inputs(c, ip=None, fields=None):
    """The case's arrays in HBM (ip / fields: dicts overriding the case's, None entries = NULL members)."""
    ip = c.ip if ip is None else ip
    fields = c.fields if fields is None else fields
    return dict(ip={k: _d(v.reshape(-1)) for k, v in ip.items() if v is not None},
                fields={k: _d(v) for k, v in fields.items() if v is not None},
                data=_d(c.data), data_off=_d(c.data_off),
                opts=None if c.opts is None else _d(c.opts), opt_off=None if c.opt_off is None else _d(c.opt_off))


def _run(c, off, fill=0xAB, tune=None, want_raw=True, inp=None, stream=None, total=None):
    """One device call over a `fill`-filled buffer of off[n] (or `total`) bytes: (buffer, raw sums or None)."""
    inp = _inputs(c) if inp is None else inp
    out = torch.full((int(off[-1]) if total is None else total,), fill, dtype=torch.uint8, device="cuda")
    raw = torch.full((c.n,), 0x5A5A, dtype=torch.int16, device="cuda") if want_raw else None
    fn = nsx.tx_ipv4_tcp_build_dev if c.ipver == 4 else nsx.tx_ipv6_tcp_build_dev
    fn(inp["ip"], inp["fields"], inp["data"], inp["data_off"], out, _d(off), opts=inp["opts"], opt_off=inp["opt_off"],
       raw=raw, stream=stream, tune=tune)
    return host(out), (u16(raw) if want_raw else None)


def _same(c, off, got, raw, want, wraw):
    if raw is not None:
        bad = np.nonzero(raw != wraw)[0]
        assert bad.size == 0, (bad[:8], raw[bad[:8]], wraw[bad[:8]])
    if not np.array_equal(got, want):
        d = np.nonzero(got != want)[0]
        i = int(np.searchsorted(np.asarray(off, np.uint64), d[0], side="right")) - 1
        raise AssertionError(f"{d.size} bytes differ, first at {d[0]} (frame {i}, byte {d[0] - int(off[i])} of "
                             f"{int(c.flen[i])}): got {got[d[:8]]}, want {want[d[:8]]}")


def _opt_list(rng, n, every=3):
    keys = sorted(_OPT_SETS)
    return [_tx.opt_bytes(rng, keys[i % len(keys)]) if i % every else b"" for i in range(n)]


def _payloads_for(rng, ipver, targets, ob):
    """Payload lengths so that frame i is targets[i] bytes long (its options' header length allowing)."""
    olen = np.array([len(b) for b in ob], np.int64)
    hdr = _tx.IPH[ipver] + 20 + olen + np.where(olen > 0, (20 + olen) % 4, 0)
    return np.maximum(np.asarray(targets, np.int64) - hdr, 0)


# ---------------------------------------------------------------- row and dword boundaries
@functools.lru_cache(maxsize=None)
def _boundary_case(ipver, opts):
    """2,003 frames in mixed order whose lengths cover the minimum frame and +1..+4, the 1 KiB row edges 1023 /
    1024 / 1025, the pipelined path's edge 2047 / 2048 / 2049 / 2052, 3073, 8960-9001, and random lengths between;
    payloads packed behind 1 lead byte with odd lengths among them, so their source alignment takes 0-3."""
    rng = np.random.default_rng(0xE0 + ipver * 2 + opts)
    n = 2003
    lo = _tx.IPH[ipver] + 20
    edges = [lo, lo + 1, lo + 2, lo + 3, lo + 4, 1023, 1024, 1025, 2047, 2048, 2049, 2052, 3073, 8960, 8961, 8963, 9001]
    targets = rng.integers(lo, 1700, n)
    targets[:len(edges) * 12] = np.tile(edges, 12)
    rng.shuffle(targets)
    ob = _opt_list(rng, n) if opts else [b""] * n
    c = _tx.Case(rng, ipver, _payloads_for(rng, ipver, targets, ob), opts=ob if opts else None, lead=1)
    if not opts:
        assert set(edges) <= set(c.flen.tolist())
    assert len(set((c.data_off[:-1] % 4).tolist())) == 4
    off = c.packed()
    want, wraw = _tx.expected(c, off, fill=0xAB)
    return c, off, want, wraw, _inputs(c)


@pytest.mark.parametrize("run_segs", [1, 16, 64])
@pytest.mark.parametrize("kernel", [0, nsx.KERNEL_BUILD_PLAIN, nsx.KERNEL_BUILD_GENERAL],
                         ids=["auto", "plain", "general"])
@pytest.mark.parametrize("opts", [False, True], ids=["noopt", "opts"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_rows_and_dword_boundaries(ipver, opts, kernel, run_segs):
    c, off, want, wraw, inp = _boundary_case(ipver, opts)
    got, raw = _run(c, off, tune=dict(kernel=kernel, run_segs=run_segs), inp=inp)
    _same(c, off, got, raw, want, wraw)


# ---------------------------------------------------------------- all-fast groups
@pytest.mark.parametrize("opt", [None, "mss", "k2len40"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_all_fast_groups(ipver, opt):
    """4,096 frames of 1480 B payloads at 4-aligned offsets in nsx_tx_layout_host's layout: every group on the
    software-pipelined fast path (1520 / 1540 B frames, two rows), without options and with 4-aligned option sets
    (the group-staged option dwords, moved up by the IP header)."""
    rng = np.random.default_rng(0xE8 + ipver)
    n = 4096
    ob = None if opt is None else [_tx.opt_bytes(rng, opt) for _ in range(n)]
    c = _tx.Case(rng, ipver, [1480] * n, opts=ob)
    if ob is not None:  # options at 4-aligned addresses too
        c.opts, c.opt_off = np.ascontiguousarray(c.opts[1:]), c.opt_off - np.uint64(1)
    off = nsx.tx_layout_host(c.data_off, c.opt_off, _tx.IPH[ipver])
    assert np.array_equal(off, c.packed())
    want, wraw = _tx.expected(c, off, fill=0xAB)
    for tune in (None, dict(run_segs=16)):
        got, raw = _run(c, off, tune=tune)
        _same(c, off, got, raw, want, wraw)


# ---------------------------------------------------------------- group tails
@pytest.mark.parametrize("run_segs", [0, 16], ids=["default", "groups16"])
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 63, 64, 65, 1000])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_group_tails(ipver, n, run_segs):
    rng = np.random.default_rng(0xF0 + n + ipver)
    lens = rng.integers(0, 2100, n)
    lens[::7] = 4 * (lens[::7] // 4)
    c = _tx.Case(rng, ipver, lens, opts=_opt_list(rng, n, every=4), lead=2)
    off = c.packed()
    want, wraw = _tx.expected(c, off, fill=0xAB)
    got, raw = _run(c, off, tune=dict(run_segs=run_segs) if run_segs else None)
    _same(c, off, got, raw, want, wraw)


# ---------------------------------------------------------------- NULL optional fields
@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_null_optional_fields(ipver):
    """NULL ident / ttl / tclass / flow build the frames of explicit 0 / 64 / 0 / 0; a NULL TCP `offset` builds
    computeOffset()'s byte 12 (tcp.go:59-66; the case's `offset` array holds exactly that); a NULL d_tcp_raw writes
    no sums and leaves the frames the same."""
    rng = np.random.default_rng(0xF8 + ipver)
    n = 300
    c = _tx.Case(rng, ipver, rng.integers(0, 2500, n), opts=_opt_list(rng, n), lead=3)
    off = c.packed()
    want, wraw = _tx.expected(c, off, fill=0xAB, ident=0, ttl=64, tclass=0, flow=0) if ipver == 6 else \
        _tx.expected(c, off, fill=0xAB, ident=0, ttl=64)
    inp = _inputs(c, ip=dict(src=c.ip["src"], dst=c.ip["dst"]), fields=dict(c.fields, offset=None))
    assert set(inp["ip"]) == {"src", "dst"} and "offset" not in inp["fields"]
    got, raw = _run(c, off, inp=inp)
    _same(c, off, got, raw, want, wraw)
    zeros = dict(src=c.ip["src"], dst=c.ip["dst"], ident=np.zeros(n, np.uint16), ttl=np.full(n, 64, np.uint8),
                 tclass=np.zeros(n, np.uint8), flow=np.zeros(n, np.uint32))
    got2, raw2 = _run(c, off, inp=_inputs(c, ip=zeros))
    assert np.array_equal(got2, got) and np.array_equal(raw2, raw)
    got3, raw3 = _run(c, off, inp=inp, want_raw=False)
    assert raw3 is None and np.array_equal(got3, got)


@pytest.mark.parametrize("shift", [1, 2, 3])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_address_arrays_at_any_alignment(ipver, shift):
    """ip.Addr.Raw() bytes are byte arrays: src / dst that do not start on a dword boundary (views `shift` bytes
    into a device buffer) build the same frames."""
    rng = np.random.default_rng(0xF9 + ipver)
    n = 200
    c = _tx.Case(rng, ipver, rng.integers(0, 1700, n), lead=1)
    off = c.packed()
    want, wraw = _tx.expected(c, off, fill=0xAB)
    inp = _inputs(c)
    for k in ("src", "dst"):
        buf = torch.zeros(inp["ip"][k].numel() + 8, dtype=torch.uint8, device="cuda")
        buf[shift:shift + inp["ip"][k].numel()] = inp["ip"][k]
        inp["ip"][k] = buf[shift:shift + inp["ip"][k].numel()]
        assert inp["ip"][k].data_ptr() % 4 == shift and inp["ip"][k].is_contiguous()
    got, raw = _run(c, off, inp=inp, tune=dict(run_segs=16))
    _same(c, off, got, raw, want, wraw)


# ---------------------------------------------------------------- gaps and sentinels
@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_gaps_and_sentinels(ipver):
    """Output slots longer than frame + padding, from a nonzero first offset, over a 0xAB buffer: only
    [frame, round_up4(frame)) of each slot is written."""
    rng = np.random.default_rng(0xFA + ipver)
    n = 700
    c = _tx.Case(rng, ipver, rng.integers(0, 2300, n), opts=_opt_list(rng, n), lead=1)
    gap = 4 * rng.integers(0, 9, n).astype(np.uint64) * (rng.random(n) < 0.5)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(np.diff(c.packed()) + gap)
    off += np.uint64(52)
    want, wraw = _tx.expected(c, off, fill=0xAB)
    assert (want[:52] == 0xAB).all()
    for tune in (None, dict(run_segs=16), dict(run_segs=16, kernel=nsx.KERNEL_BUILD_PLAIN)):
        got, raw = _run(c, off, tune=tune)
        _same(c, off, got, raw, want, wraw)


# ---------------------------------------------------------------- over-long frames
@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_over_long_frames_are_not_built(ipver):
    """Among 100 small frames, one whose TCP part is one byte more than the IP length field carries (IPv4 wire
    65516, IPv6 65536) and one that just fits (65515 / 65535): the over-long slot keeps its 0xAB bytes and gets raw
    sum 0; every other frame, the longest included, is exact."""
    rng = np.random.default_rng(0xFC + ipver)
    top = _tx.WIRE_MAX[ipver]
    lens = rng.integers(0, 600, 102)
    lens[40], lens[71] = top + 1 - 20, top - 20
    c = _tx.Case(rng, ipver, lens)
    assert int(c.wire[40]) == top + 1 and int(c.wire[71]) == top
    off = c.packed()
    want, wraw = _tx.expected(c, off, fill=0xAB)
    assert wraw[40] == 0 and (want[int(off[40]):int(off[41])] == 0xAB).all() and (wraw[np.arange(102) != 40] != 0).all()
    for tune in (None, dict(run_segs=16)):
        got, raw = _run(c, off, tune=tune)
        _same(c, off, got, raw, want, wraw)


# ---------------------------------------------------------------- closing the loop on the device
@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_frames_pass_the_receive_kernel(ipver):
    """10,000 frames with every length a multiple of 4 in packed layout: the build's d_out / d_out_off go straight
    into the fused receive pass, which finds every frame valid (mask all ones, ip_raw and tcp_raw 0xFFFF); after one
    bit of one frame's payload is flipped exactly that frame's mask bit clears."""
    rng = np.random.default_rng(0xFE + ipver)
    n = 10_000
    keys = ["mss", "nop_nop_k2len10", "k2len40"]  # 4-aligned headers
    ob = [_tx.opt_bytes(rng, keys[i % 3]) if i % 5 == 0 else b"" for i in range(n)]
    c = _tx.Case(rng, ipver, 4 * rng.integers(0, 500, n), opts=ob)
    off = c.packed()
    assert not (c.flen % 4).any()
    inp = _inputs(c)
    d_off = _d(off)
    d_out = torch.full((int(off[-1]),), 0xAB, dtype=torch.uint8, device="cuda")
    fn = nsx.tx_ipv4_tcp_build_dev if ipver == 4 else nsx.tx_ipv6_tcp_build_dev
    fn(inp["ip"], inp["fields"], inp["data"], inp["data_off"], d_out, d_off, opts=inp["opts"], opt_off=inp["opt_off"])

    def verify():
        tcp_raw = torch.empty(n, dtype=torch.int16, device="cuda")
        if ipver == 4:
            ip_raw = torch.empty(n, dtype=torch.int16, device="cuda")
            mask = nsx.rx_ipv4_tcp_verify_dev(d_out, d_off, ip_raw=ip_raw, tcp_raw=tcp_raw)
            return host(mask).view(np.uint64), u16(tcp_raw), u16(ip_raw)
        mask = nsx.rx_ipv6_tcp_verify_dev(d_out, d_off, tcp_raw=tcp_raw)
        return host(mask).view(np.uint64), u16(tcp_raw), None

    ones = np.packbits(np.ones(n, np.uint8), bitorder="little")
    ones = np.concatenate([ones, np.zeros(-ones.size % 8, np.uint8)]).view(np.uint64)
    mask, tcp_raw, ip_raw = verify()
    assert np.array_equal(mask, ones)
    assert (tcp_raw == 0xFFFF).all() and (ip_raw is None or (ip_raw == 0xFFFF).all())
    victim = int(np.nonzero(c.flen > _tx.IPH[ipver] + 64)[0][1234])
    d_out[int(off[victim]) + int(c.flen[victim]) - 2] ^= 0x10
    mask, tcp_raw, ip_raw = verify()
    want = ones.copy()
    want[victim // 64] ^= np.uint64(1) << np.uint64(victim % 64)
    assert np.array_equal(mask, want)
    assert np.array_equal(np.nonzero(tcp_raw != 0xFFFF)[0], [victim])


# ---------------------------------------------------------------- host calls
@functools.lru_cache(maxsize=None)
def _host_case(ipver):
    """20,000 mixed frames, ~30 MB: payloads of 0-2900 B, every 97th a 8940 B jumbo, every third frame with options."""
    rng = np.random.default_rng(0x100 + ipver)
    n = 20_000
    lens = rng.integers(0, 2901, n)
    lens[::97] = 8940
    c = _tx.Case(rng, ipver, lens, opts=_opt_list(rng, n), lead=7)
    off = c.packed()
    want, wraw = _tx.expected(c, off, fill=0xAB)
    dgot, draw = _run(c, off)
    return c, off, want, wraw, dgot, draw


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("mem", ["pageable", "pinned"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_host_calls(ipver, mem, shards):
    """nsx_tx_ipv4_tcp_build_host / nsx_tx_ipv6_tcp_build_host from and to pageable or pinned memory, 1 or 3 shards
    on the device: frames and raw sums equal tests/_tx.py and the device call over the same inputs."""
    c, off, want, wraw, dgot, draw = _host_case(ipver)
    fn = nsx.tx_ipv4_tcp_build_host if ipver == 4 else nsx.tx_ipv6_tcp_build_host
    kw = dict(out_off=off, opts=c.opts, opt_off=c.opt_off, tune=dict(shards_per_device=shards))
    if mem == "pinned":
        dp, op = nsx.PinnedBuffer(c.data.nbytes), nsx.PinnedBuffer(int(off[-1]))
        dp.array[:] = c.data
        op.array[:] = 0xAB
        got, raw = fn(c.ip, c.fields, dp.array, c.data_off, out=op.array, **kw)
        got = got.copy()
        dp.free()
        op.free()
    else:
        got, raw = fn(c.ip, c.fields, c.data, c.data_off, out=np.full(int(off[-1]), 0xAB, np.uint8), **kw)
    _same(c, off, got, raw, want, wraw)
    assert np.array_equal(got, dgot) and np.array_equal(raw, draw)


@functools.lru_cache(maxsize=None)
def _small_host_case(ipver):
    """50 frames, options on every third: payloads of 0-1600 B with a 0, a 1 and a 8940 B one among them; packed
    slots, and slots with 4-byte-multiple gaps. Expected frames over an 0xAB-filled buffer for both."""
    rng = np.random.default_rng(0x110 + ipver)
    n = 50
    lens = rng.integers(0, 1601, n)
    lens[[0, 1, 2, 31]] = [0, 1, 1480, 8940]
    c = _tx.Case(rng, ipver, lens, opts=_opt_list(rng, n), lead=7)
    packed = c.packed()
    gap = 4 * rng.integers(0, 9, n).astype(np.uint64) * (rng.random(n) < 0.3)
    wide = np.zeros(n + 1, np.uint64)
    wide[1:] = np.cumsum(np.diff(packed) + gap)
    assert gap.any()
    return c, [(off, *_tx.expected(c, off, fill=0xAB)) for off in (packed, wide)]


@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("mem", ["pageable", "pinned"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_host_calls_small_chunks(ipver, mem, shards):
    """The transmit host calls cut into 2048 B chunks (nsx_tune.chunk_bytes): ~30 chunks on one shard, so both stream
    slots are reused many times, the jumbo frame a chunk of its own; packed and gapped layouts over a sentinel-filled
    output, with and without raw sums, and once in a single chunk. Every frame byte, gap byte and raw sum against
    tests/_tx.py."""
    c, layouts = _small_host_case(ipver)
    fn = nsx.tx_ipv4_tcp_build_host if ipver == 4 else nsx.tx_ipv6_tcp_build_host
    dp = nsx.PinnedBuffer(c.data.nbytes) if mem == "pinned" else None
    data = c.data
    if dp is not None:
        dp.array[:] = c.data
        data = dp.array
    for off, want, wraw in layouts:
        op = nsx.PinnedBuffer(int(off[-1])) if mem == "pinned" else None
        for want_raw, chunk in ((True, 2048), (False, 2048), (True, 0)):
            out = op.array if op is not None else np.empty(int(off[-1]), np.uint8)
            out[:] = 0xAB
            got, raw = fn(c.ip, c.fields, data, c.data_off, out_off=off, opts=c.opts, opt_off=c.opt_off, out=out,
                          want_raw=want_raw, tune=dict(shards_per_device=shards, chunk_bytes=chunk))
            assert (raw is not None) == want_raw
            _same(c, off, got.copy(), raw, want, wraw)
        if op is not None:
            op.free()
    if dp is not None:
        dp.free()


@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_host_more_gpus_than_present_is_enodev(ipver):
    rng = np.random.default_rng(0x104 + ipver)
    c = _tx.Case(rng, ipver, [100, 200, 300])
    fn = nsx.tx_ipv4_tcp_build_host if ipver == 4 else nsx.tx_ipv6_tcp_build_host
    before = torch.cuda.current_device()
    with pytest.raises(nsx.NsxError) as e:
        fn(c.ip, c.fields, c.data, c.data_off, num_gpus=nsx.device_count() + 1)
    assert e.value.code == nsx.NSX_ENODEV
    assert torch.cuda.current_device() == before
    got, raw = fn(c.ip, c.fields, c.data, c.data_off, num_gpus=nsx.device_count())
    want, wraw = _tx.expected(c, c.packed())
    _same(c, c.packed(), got, raw, want, wraw)


# ---------------------------------------------------------------- graph capture
@pytest.mark.parametrize("ipver", [4, 6])
def test_tx_device_call_captures_into_a_graph(ipver):
    """The device call allocates nothing and never synchronises: captured with torch.cuda.graph on a side stream and
    replayed once, it builds the exact frames."""
    rng = np.random.default_rng(0x108 + ipver)
    n = 1500
    c = _tx.Case(rng, ipver, rng.integers(0, 2200, n), opts=_opt_list(rng, n), lead=1)
    off = c.packed()
    want, wraw = _tx.expected(c, off, fill=0xAB)
    inp = _inputs(c)
    d_off = _d(off)
    out = torch.full((int(off[-1]),), 0xAB, dtype=torch.uint8, device="cuda")
    raw = torch.zeros(n, dtype=torch.int16, device="cuda")
    fn = nsx.tx_ipv4_tcp_build_dev if ipver == 4 else nsx.tx_ipv6_tcp_build_dev
    # a first call outside capture (library and device-info setup), into a buffer of its own
    fn(inp["ip"], inp["fields"], inp["data"], inp["data_off"], torch.empty_like(out), d_off, opts=inp["opts"],
       opt_off=inp["opt_off"])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn(inp["ip"], inp["fields"], inp["data"], inp["data_off"], out, d_off, opts=inp["opts"],
           opt_off=inp["opt_off"], raw=raw)
    torch.cuda.synchronize()
    assert (host(out) == 0xAB).all()  # capture ran nothing
    g.replay()
    _same(c, off, host(out), u16(raw), want, wraw)
