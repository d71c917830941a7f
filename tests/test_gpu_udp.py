"""The UDP passes on the GPU (nsx_udp_tx_* / nsx_udp_uso_* / nsx_udp_rx_*): every output byte — untouched bytes and
padding included — every raw sum and every mask bit against the CPU restatement tests/_udp.py (held to nsx.csum16 and
the oracle by tests/test_udp_abi.py). Bit-exact throughout. blocks_per_cu 1 with run_segs 1, 2 and 64 reaches the
wave's second task and a ragged last group with about a thousand small frames."""
import ctypes
import functools

import numpy as np
import pytest

import _far
import _tx
import _udp
from _gpu import dev, host, mask_words, setup_gpu, torch, u16, nsx

pytestmark = pytest.mark.gpu

FILL = 0xAB
_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
           np.dtype(np.uint64): np.int64}
# payload lengths: the dword edges, the per-lane path's limit (a 256 B payload on transmit, a 256 B datagram on receive),
# the first and second 1 KiB row of the payload and of the frame, one MTU
LENS = {4: [0, 1, 2, 3, 4, 7, 8, 15, 16, 17, 247, 248, 249, 255, 256, 257, 995, 996, 997, 1023, 1024, 1025, 1472, 2019, 2020, 2021, 2047, 2048, 2049],
        6: [0, 1, 2, 3, 4, 7, 8, 15, 16, 17, 247, 248, 249, 255, 256, 257, 975, 976, 977, 1023, 1024, 1025, 1472, 1999, 2000, 2001, 2047, 2048, 2049]}
TUNES = [dict(blocks_per_cu=1, run_segs=1), dict(blocks_per_cu=1, run_segs=2), dict(blocks_per_cu=1, run_segs=64), None]
TUNE_IDS = ["segs1", "segs2", "segs64", "default"]


def setup_module(module):
    setup_gpu()


def _d(a):
    a = np.ascontiguousarray(a)
    return dev(a.view(_SIGNED[a.dtype]))


def _soa(c, null=()):
    return ({k: _d(v.reshape(-1)) for k, v in c.ip.items() if k not in null}, {k: _d(v) for k, v in c.ports.items()})


def _tx_run(c, off, tune=None, flags=0, want_raw=True, null=(), total=None, data=None):
    """One transmit call over a FILL-filled buffer of off[n] (or `total`) bytes: (buffer, raw sums or None)."""
    ip, ports = _soa(c, null)
    out = torch.full((int(off[-1]) if total is None else total,), FILL, dtype=torch.uint8, device="cuda")
    raw = torch.full((c.n,), 0x5A5A, dtype=torch.int16, device="cuda") if want_raw else None
    fn = nsx.udp_tx_ipv4_build_dev if c.ipver == 4 else nsx.udp_tx_ipv6_build_dev
    fn(ip, ports, _d(c.data) if data is None else data, _d(c.data_off), out, _d(off), flags=flags, raw=raw, tune=tune)
    return host(out), (u16(raw) if want_raw else None)


def _uso_run(b, off=None, tune=None, flags=0, want_raw=True, null=(), seg=None, total=None):
    off = b.off if off is None else off
    ip, ports = _soa(b.sup, null)
    out = torch.full((int(off[-1]) if total is None else total,), FILL, dtype=torch.uint8, device="cuda")
    raw = torch.full((b.nf,), 0x5A5A, dtype=torch.int16, device="cuda") if want_raw else None
    fn = nsx.udp_uso_ipv4_build_dev if b.ipver == 4 else nsx.udp_uso_ipv6_build_dev
    fn(ip, ports, _d(b.sup.data), _d(b.sup.data_off), _d(b.gso), _d(b.first), _d(b.seg if seg is None else seg), out,
       _d(off), flags=flags, raw=raw, tune=tune)
    return host(out), (u16(raw) if want_raw else None)


def _same(off, got, raw, want, wraw, what=""):
    if raw is not None:
        bad = np.nonzero(raw != wraw)[0]
        assert bad.size == 0, (what, bad[:8], raw[bad[:8]], wraw[bad[:8]])
    if not np.array_equal(got, want):
        d = np.nonzero(got != want)[0]
        i = int(np.searchsorted(np.asarray(off, np.uint64), d[0], side="right")) - 1
        raise AssertionError(f"{what}: {d.size} bytes differ, first at {d[0]} (frame {i}, byte {d[0] - int(off[i])}): "
                             f"got {got[d[:8]]}, want {want[d[:8]]}")


def _rx_run(ipver, buf, offs, tune=None, want_raw=True):
    n = len(offs) - 1
    mask = torch.full(((n + 63) // 64,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    ipr = torch.full((n,), 0x5A5A, dtype=torch.int16, device="cuda") if want_raw else None
    udr = torch.full((n,), 0x5A5A, dtype=torch.int16, device="cuda") if want_raw else None
    dbuf = buf if isinstance(buf, torch.Tensor) else dev(buf)
    if ipver == 4:
        nsx.udp_rx_ipv4_verify_dev(dbuf, _d(np.asarray(offs, np.uint64)), mask=mask, ip_raw=ipr, udp_raw=udr, tune=tune)
    else:
        nsx.udp_rx_ipv6_verify_dev(dbuf, _d(np.asarray(offs, np.uint64)), mask=mask, udp_raw=udr, tune=tune)
    return host(mask).view(np.uint64), (u16(ipr) if want_raw else None), (u16(udr) if want_raw else None)


def _rx_same(ipver, got, want, names=None, what=""):
    mask, ipr, udr = got
    valid, wipr, wudr = want
    if udr is not None:
        bad = np.nonzero(udr != wudr)[0]
        assert bad.size == 0, (what, "udp_raw", bad[:8], [names[i] for i in bad[:8]] if names else None, udr[bad[:8]],
                               wudr[bad[:8]])
        if ipver == 4:
            bad = np.nonzero(ipr != wipr)[0]
            assert bad.size == 0, (what, "ip_raw", bad[:8], ipr[bad[:8]], wipr[bad[:8]])
        else:
            assert (ipr == 0x5A5A).all()  # IPv6 has no header checksum: nothing written
    wm = mask_words(valid)
    if not np.array_equal(mask, wm):
        gotb = np.unpackbits(mask.view(np.uint8), bitorder="little")[:valid.size].astype(bool)
        bad = np.nonzero(gotb != valid)[0]
        raise AssertionError((what, "mask", bad[:8], [names[i] for i in bad[:8]] if names else None, mask, wm))


# ---------------------------------------------------------------- transmit: lengths, alignments, groups
@functools.lru_cache(maxsize=None)
def _len_case(ipver, lead):
    rng = np.random.default_rng([0x0DA0, ipver, lead])
    lens = LENS[ipver] + [_udp.PAY_MAX[ipver], _udp.PAY_MAX[ipver] + 1] + LENS[ipver][::-1]
    c = _udp.Case(rng, ipver, lens, lead=lead)
    off = c.packed()
    want, wraw = _udp.expected(c, off, fill=FILL)
    k = len(LENS[ipver])
    assert wraw[k] != 0 and wraw[k + 1] == 0  # the last built frame and the first one not built
    assert (want[int(off[k + 1]):int(off[k + 2])] == FILL).all()
    return c, off, want, wraw


@pytest.mark.parametrize("tune", TUNES, ids=TUNE_IDS)
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_tx_lengths_and_source_alignment(ipver, lead, tune):
    """Every payload length class at every source alignment (packed payloads of odd lengths behind `lead` bytes take
    all four), 65507 / 65527 built and one byte more not built: nothing written for it, raw 0."""
    c, off, want, wraw = _len_case(ipver, lead)
    assert len(set((c.data_off[:-1] % 4).tolist())) == 4
    got, raw = _tx_run(c, off, tune=tune)
    _same(off, got, raw, want, wraw, "tx")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("tune", TUNES, ids=TUNE_IDS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300, "second_trip"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_tx_batch_sizes(ipver, n, tune):
    """n = 1, 63, 64, 65 and 300 frames, and 70 frames more than one trip of a one-block-per-CU grid holds: the
    wave's second task and a ragged last group."""
    if n == "second_trip":
        n = _cus() * 4 * min((tune or {}).get("run_segs", 1), 2) + 70
    rng = np.random.default_rng([0x0DA1, ipver, n])
    c = _udp.Case(rng, ipver, rng.integers(0, 90, n), lead=int(rng.integers(4)))
    off = c.packed()
    want, wraw = _udp.expected(c, off, fill=FILL)
    got, raw = _tx_run(c, off, tune=tune)
    _same(off, got, raw, want, wraw, "tx")


@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_tx_checksum_zero_is_sent_as_ffff(ipver):
    """One frame per length class crafted so that raw == 0xFFFF (an aligned payload word, and again the two bytes at
    an odd payload offset): the stored field is 0xFFFF, never 0x0000."""
    rng = np.random.default_rng([0x0DA2, ipver])
    classes = [2, 3, 17, 100, 997, 1472, 2021, 9000]
    lens = [x for L in classes for x in (L, L + 1)]
    c = _udp.Case(rng, ipver, lens, lead=1)
    for k, L in enumerate(classes):
        _udp.craft_ffff(c, 2 * k, (L - 2) & ~1 if L < 100 else 2 * int(rng.integers(L // 2 - 1)))
        _udp.craft_ffff(c, 2 * k + 1, 1 if L < 100 else 1 + 2 * int(rng.integers(L // 2 - 1)))
    off = c.packed()
    want, wraw = _udp.expected(c, off, fill=FILL)
    assert (wraw == 0xFFFF).all()
    h = _udp.IPH[ipver]
    for tune in TUNES:
        got, raw = _tx_run(c, off, tune=tune)
        for i in range(c.n):
            o = int(off[i]) + h + 6
            assert bytes(got[o:o + 2]) == b"\xff\xff", (i, tune)
        _same(off, got, raw, want, wraw, "crafted")


def test_udp_tx_no_csum_ipv4():
    """NSX_UDP_NO_CSUM: the field is 0 in every frame, the raw sums are still reported; IPv6 refuses the flag."""
    c, off, _, wraw = _len_case(4, 1)
    want, wraw2 = _udp.expected(c, off, fill=FILL, flags=_udp.NO_CSUM)
    assert np.array_equal(wraw, wraw2)
    got, raw = _tx_run(c, off, flags=nsx.UDP_NO_CSUM)
    _same(off, got, raw, want, wraw, "no_csum")
    assert bytes(got[26:28]) == b"\0\0"
    c6, off6, _, _ = _len_case(6, 1)
    with pytest.raises(nsx.NsxError) as e:
        _tx_run(c6, off6, flags=nsx.UDP_NO_CSUM)
    assert e.value.code == nsx.NSX_EINVAL


@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_tx_optional_arguments(ipver):
    """d_udp_raw NULL; the optional nsx_ip_hdr_soa members NULL (ident 0, ttl 64, tclass 0, flow 0); non-packed
    d_out_off with gaps, which stay FILL, in a buffer longer than the last slot."""
    rng = np.random.default_rng([0x0DA3, ipver])
    n = 150
    c = _udp.Case(rng, ipver, rng.integers(0, 1600, n), lead=3)
    off = c.packed()
    want, wraw = _udp.expected(c, off, fill=FILL)
    got, raw = _tx_run(c, off, want_raw=False)
    _same(off, got, raw, want, wraw, "raw NULL")
    null = ("ident", "ttl", "tclass", "flow")
    want, wraw = _udp.expected(c, off, fill=FILL, null=null)
    got, raw = _tx_run(c, off, null=null)
    _same(off, got, raw, want, wraw, "NULL members")
    for one in null:
        want, wraw = _udp.expected(c, off, fill=FILL, null=(one,))
        got, raw = _tx_run(c, off, null=(one,))
        _same(off, got, raw, want, wraw, one)
    gaps = np.zeros(n + 1, np.uint64)
    gaps[1:] = np.cumsum(np.diff(off) + (rng.integers(0, 9, n) * 4).astype(np.uint64))
    gaps += np.uint64(8)
    total = int(gaps[-1]) + 40
    want, wraw = _udp.expected(c, gaps, fill=FILL, total=total)
    got, raw = _tx_run(c, gaps, total=total, tune=TUNES[1])
    _same(gaps, got, raw, want, wraw, "gaps")
    assert (got[:8] == FILL).all() and (got[-40:] == FILL).all()


@pytest.mark.parametrize("ipver", [4, 6])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_udp_tx_address_arrays_at_any_alignment(ipver, shift):
    rng = np.random.default_rng([0x0DA4, ipver, shift])
    n = 70
    c = _udp.Case(rng, ipver, rng.integers(0, 300, n))
    off = c.packed()
    want, wraw = _udp.expected(c, off, fill=FILL)
    ip, ports = _soa(c)
    for k in ("src", "dst"):
        t = torch.zeros(ip[k].numel() + 4, dtype=torch.uint8, device="cuda")
        t[shift:shift + ip[k].numel()] = ip[k]
        ip[k] = t[shift:shift + ip[k].numel()]
    out = torch.full((int(off[-1]),), FILL, dtype=torch.uint8, device="cuda")
    raw = torch.zeros(n, dtype=torch.int16, device="cuda")
    fn = nsx.udp_tx_ipv4_build_dev if ipver == 4 else nsx.udp_tx_ipv6_build_dev
    fn(ip, ports, _d(c.data), _d(c.data_off), out, _d(off), raw=raw)
    _same(off, host(out), u16(raw), want, wraw, "unaligned addresses")


# ---------------------------------------------------------------- segmentation offload
def _cut_lengths(gso):
    return sorted({0, 1, gso - 1, gso, gso + 1, 3 * gso - 1, 3 * gso, 3 * gso + 1})


@functools.lru_cache(maxsize=None)
def _cut_case(ipver, gso):
    rng = np.random.default_rng([0x0DB0, ipver, gso])
    lens = np.array(_cut_lengths(gso) * 3)
    rng.shuffle(lens)
    b = _udp.Batch(rng, ipver, lens, gso, lead=1)
    multi = np.nonzero(np.diff(b.first) >= 3)[0]  # the ident wraps inside these super-datagrams
    b.sup.ip["ident"][multi[0::2]], b.sup.ip["ident"][multi[1::2]] = 0xFFFF, 0xFFFE
    want, wraw, c = _udp.uso_expected(b, fill=FILL)
    return b, c, want, wraw


@pytest.mark.parametrize("tune", TUNES, ids=TUNE_IDS)
@pytest.mark.parametrize("gso", [1, 7, 512, 1472])
@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_uso_cut_points(ipver, gso, tune):
    """Super-datagrams of 0, 1, gso - 1, gso, gso + 1, 3·gso ± 1 and 3·gso bytes in mixed order behind one lead byte,
    idents that wrap at 0xFFFF; the layout helpers give the model's map; and the same bytes come out of
    nsx_udp_tx_* over the expanded batch."""
    b, c, want, wraw = _cut_case(ipver, gso)
    first = nsx.tso_count_host(b.sup.data_off, b.gso)
    seg, off = nsx.udp_uso_layout_host(b.sup.data_off, b.gso, first, _udp.IPH[ipver])
    assert np.array_equal(first, b.first) and np.array_equal(seg, b.seg) and np.array_equal(off, b.off)
    if ipver == 4:
        ids = c.ip["ident"].astype(np.int64)
        assert ((ids[1:] == 0) & (ids[:-1] == 0xFFFF) & (b.seg[1:] == b.seg[:-1])).any()
    got, raw = _uso_run(b, tune=tune)
    _same(b.off, got, raw, want, wraw, "uso")
    got2, raw2 = _tx_run(c, b.off, tune=tune)
    assert np.array_equal(got, got2) and np.array_equal(raw, raw2)


@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_uso_options_and_second_trip(ipver):
    """More frames than one trip of a one-block-per-CU grid (run_segs 1), groups that straddle super-datagrams;
    NO_CSUM (IPv4), NULL ident / ttl / tclass / flow, d_udp_raw NULL, slots with gaps."""
    rng = np.random.default_rng([0x0DB1, ipver])
    lens = rng.integers(100, 360, 2 + _cus())  # at least 6 frames each
    lens[::9] = 0
    b = _udp.Batch(rng, ipver, lens, rng.integers(4, 20, lens.size), lead=2)
    assert b.nf > _cus() * 4
    want, wraw, _ = _udp.uso_expected(b, fill=FILL)
    got, raw = _uso_run(b, tune=TUNES[0])
    _same(b.off, got, raw, want, wraw, "second trip")
    null = ("ident", "ttl", "tclass", "flow")
    flags = _udp.NO_CSUM if ipver == 4 else 0
    gaps = np.zeros(b.nf + 1, np.uint64)
    gaps[1:] = np.cumsum(np.diff(b.off) + (rng.integers(0, 5, b.nf) * 4).astype(np.uint64))
    total = int(gaps[-1]) + 16
    want, wraw, _ = _udp.uso_expected(b, off=gaps, fill=FILL, flags=flags, null=null, total=total)
    got, raw = _uso_run(b, off=gaps, flags=flags, null=null, total=total, tune=TUNES[1])
    _same(gaps, got, raw, want, wraw, "flags, NULL members, gaps")
    got, raw = _uso_run(b, off=gaps, flags=flags, null=null, total=total, want_raw=False)
    _same(gaps, got, raw, want, wraw, "raw NULL")


@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_uso_lying_frame_map_stays_inside_the_super_datagram(ipver):
    """frame_seg lies about one frame at a time: the frame is built from the super-datagram it names, its slice
    clamped to that one's own range (empty where j·gso passes it) — the model's expansion with the same map. d_data
    holds nothing behind the last super-datagram's bytes."""
    rng = np.random.default_rng([0x0DB2, ipver])
    b = _udp.Batch(rng, ipver, [0, 1, 20, 21, 22, 100, 3000], [7, 7, 7, 7, 7, 7, 1472], lead=2)
    b.sup.data = np.ascontiguousarray(b.sup.data[:int(b.sup.data_off[-1])])
    for f, s in ((3, 5), (3, 1), (0, 6), (b.nf - 1, 2), (b.nf - 1, 0), (12, 6), (13, 5)):
        lie = b.seg.copy()
        lie[f] = s
        want, wraw, c = _udp.uso_expected(b, fill=FILL, seg=lie)
        lo, hi = int(b.sup.data_off[s]), int(b.sup.data_off[s + 1])
        assert lo <= int(c.lo[f]) <= int(c.hi[f]) <= hi and int(c.plen[f]) <= int(b.gso[s])
        # the slot the true map laid out holds whatever the lie builds: the lie's slice is never longer
        assert int(c.plen[f]) <= int(np.diff(b.off)[f]) - _udp.IPH[ipver] - 8
        for tune in (None, TUNES[0]):
            got, raw = _uso_run(b, seg=lie, tune=tune)
            _same(b.off, got, raw, want, wraw, f"frame {f} claims {s}")


# ---------------------------------------------------------------- receive
@functools.lru_cache(maxsize=None)
def _edge_batch(ipver, n):
    edge = _udp.rx_edge_frames(ipver)
    pick = [edge[i % len(edge)] for i in range(n)] if n > 1 else [edge[3]]
    if n >= 64:  # the 64 KiB frame once, the word's other frames around it
        big = [i for i, (name, _) in enumerate(pick) if name == "frame_64k"]
        pick = [p for i, p in enumerate(pick) if i not in big[1:]] + [edge[0]] * len(big[1:])
    rng = np.random.default_rng([0x0DC0, ipver, n])
    buf, offs = _udp.concat([f for _, f in pick], lead=1, rng=rng)
    return [name for name, _ in pick], buf, offs, _udp.rx_expected(ipver, buf, offs)


@pytest.mark.parametrize("tune", [None, dict(blocks_per_cu=1, run_segs=1), dict(blocks_per_cu=1, run_segs=7)],
                         ids=["default", "step1", "step7"])
@pytest.mark.parametrize("n", [1, 64, 65, 129])
@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_rx_edge_batch(ipver, n, tune):
    """The edge batch behind an odd lead byte: valid frames; one wrong payload byte; a wrong header checksum; field 0
    (accepted on IPv4 with any raw, rejected on IPv6); field 0xFFFF on a crafted frame; U = P; U < P with junk
    padding; U < 8; U > P; protocol 6; fragments; a length mismatch; IHL 6 with options; IHL < 5; the wrong version;
    frames of 0, 27, 28 / 47, 48 bytes; a 64 KiB frame. n = 1, 64, 65, 129: the last mask word's high bits are 0."""
    names, buf, offs, want = _edge_batch(ipver, n)
    if n >= 64:
        assert len(set(names)) == len(_udp.rx_edge_frames(ipver)) and want[0].any() and not want[0].all()
    got = _rx_run(ipver, buf, offs, tune=tune)
    _rx_same(ipver, got, want, names)
    if n % 64:
        assert int(got[0][-1]) >> (n % 64) == 0
    got = _rx_run(ipver, buf, offs, tune=tune, want_raw=False)
    _rx_same(ipver, got, want, names, "raws NULL")


@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_rx_second_trip(ipver):
    """More mask words than one trip of a one-block-per-CU grid holds."""
    rng = np.random.default_rng([0x0DC1, ipver])
    n = 64 * (_cus() * 4 + 3) + 5
    c = _udp.Case(rng, ipver, rng.integers(0, 24, n), lead=1)
    fr, _ = _udp.frames(c)
    for i in range(0, n, 7):
        fr[i] = _udp.corrupt(rng, fr[i], ipver, _udp.CORRUPTIONS[(i // 7) % len(_udp.CORRUPTIONS)])
    buf, offs = _udp.concat(fr, lead=3, rng=rng)
    want = _udp.rx_expected(ipver, buf, offs)
    _rx_same(ipver, _rx_run(ipver, buf, offs, tune=dict(blocks_per_cu=1)), want)


# ---------------------------------------------------------------- guard bytes
class _HipBuf:
    """A device allocation of its own (hipMalloc, a multiple of 2 MiB) with `data` in its last bytes."""
    hip = None

    def __init__(self, data, fill=None):
        if _HipBuf.hip is None:
            _HipBuf.hip = ctypes.CDLL("libamdhip64.so")
        data = np.ascontiguousarray(data)
        self.n = data.nbytes
        self.size = max(2 << 20, (self.n + (2 << 20) - 1) & ~((2 << 20) - 1))
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(self.size)) == 0
        self.base = p.value
        self.ptr = ctypes.c_void_p(self.base + self.size - self.n)  # the data ends where the allocation ends
        if fill is not None:
            assert self.hip.hipMemset(ctypes.c_void_p(self.base), fill, ctypes.c_size_t(self.size)) == 0
        if self.n:
            assert self.hip.hipMemcpy(self.ptr, data.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(self.n), 1) == 0

    def get(self):
        out = np.empty(self.n, np.uint8)
        assert self.hip.hipDeviceSynchronize() == 0
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), self.ptr, ctypes.c_size_t(self.n), 2) == 0
        return out

    def free(self):
        self.hip.hipFree(ctypes.c_void_p(self.base))


@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_batches_at_the_very_end_of_their_allocations(ipver):
    """Transmit: the payloads end with d_data's allocation (every tail length 0-3 past a dword over the batches) and
    the frames end with d_out's. Receive: the last frame ends with d_base's allocation. The C calls take the raw pointers; every result equals the model's."""
    L = nsx.lib()
    rng = np.random.default_rng([0x0DD0, ipver])
    bufs = []
    try:
        for tail in range(4):
            n = 130
            lens = rng.integers(0, 300, n)
            lens[-1] = 4 * int(lens[-1] // 4) + tail + (4 if tail == 0 else 0)
            c = _udp.Case(rng, ipver, lens, lead=1)
            data = c.data[:int(c.data_off[-1])]
            off = c.packed()
            want, wraw = _udp.expected(c, off, fill=FILL)
            d_data, d_out = _HipBuf(data), _HipBuf(np.full(int(off[-1]), FILL, np.uint8))
            bufs += [d_data, d_out]
            ip, ports = _soa(c)
            ipsoa = nsx.IpHdrSoA(*[ctypes.c_void_p(ip[k].data_ptr()) for k in nsx.IP_FIELDS])
            usoa = nsx.UdpHdrSoA(*[ctypes.c_void_p(ports[k].data_ptr()) for k in nsx.UDP_FIELDS])
            doff, ooff = _d(c.data_off), _d(off)
            raw = torch.zeros(n, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            fn = getattr(L, f"nsx_udp_tx_ipv{ipver}_build_dev")
            rc = fn(ctypes.byref(ipsoa), ctypes.byref(usoa), d_data.ptr, ctypes.c_void_p(doff.data_ptr()), data.size, n, 0,
                    d_out.ptr, ctypes.c_void_p(ooff.data_ptr()), ctypes.c_void_p(raw.data_ptr()), None)
            assert rc == 0
            _same(off, d_out.get(), u16(raw), want, wraw, f"tx tail {tail}")
            # receive over the same frames
            fr, _ = _udp.frames(c)
            fr[5] = _udp.corrupt(rng, fr[5], ipver, "payload_byte")
            buf, offs = _udp.concat(fr, lead=1)
            wv, wipr, wudr = _udp.rx_expected(ipver, buf, offs)
            d_base = _HipBuf(buf)
            bufs.append(d_base)
            assert (d_base.base + d_base.size) % 4 == 0
            mask = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
            ipr = torch.zeros(n, dtype=torch.int16, device="cuda")
            udr = torch.zeros(n, dtype=torch.int16, device="cuda")
            doffs = _d(offs)
            torch.cuda.synchronize()
            fn = getattr(L, f"nsx_udp_rx_ipv{ipver}_verify_dev")
            args = [d_base.ptr, ctypes.c_void_p(doffs.data_ptr()), n, ctypes.c_void_p(mask.data_ptr())]
            args += [ctypes.c_void_p(ipr.data_ptr())] if ipver == 4 else []
            assert fn(*args, ctypes.c_void_p(udr.data_ptr()), None) == 0
            got = (host(mask).view(np.uint64), u16(ipr) if ipver == 4 else np.full(n, 0x5A5A, np.uint16), u16(udr))
            _rx_same(ipver, got, (wv, wipr, wudr), what=f"rx tail {tail}")
    finally:
        torch.cuda.synchronize()
        for b in bufs:
            b.free()


# ---------------------------------------------------------------- round trip and separation
@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_uso_frames_pass_the_udp_receive_pass_and_no_other(ipver):
    """USO -> nsx_udp_rx_*: every frame valid, with the checksum on and (IPv4) with NO_CSUM. The TCP receive pass over
    the UDP frames and the UDP receive pass over nsx_tx_*_tcp_build_dev frames give all-zero masks. Payload lengths
    are multiples of 4, so the packed d_out_off is directly the receive pass's d_offsets."""
    rng = np.random.default_rng([0x0DE0, ipver])
    b = _udp.Batch(rng, ipver, 4 * rng.integers(0, 1200, 40), 4 * rng.integers(1, 370, 40))
    ip, ports = _soa(b.sup)
    out = torch.zeros(int(b.off[-1]), dtype=torch.uint8, device="cuda")
    fn = nsx.udp_uso_ipv4_build_dev if ipver == 4 else nsx.udp_uso_ipv6_build_dev
    rx = nsx.udp_rx_ipv4_verify_dev if ipver == 4 else nsx.udp_rx_ipv6_verify_dev
    tcp_rx = nsx.rx_ipv4_tcp_verify_dev if ipver == 4 else nsx.rx_ipv6_tcp_verify_dev
    full = mask_words(np.ones(b.nf, bool))
    d_off = _d(b.off)
    for flags in ((0, nsx.UDP_NO_CSUM) if ipver == 4 else (0,)):
        raw = torch.zeros(b.nf, dtype=torch.int16, device="cuda")
        fn(ip, ports, _d(b.sup.data), _d(b.sup.data_off), _d(b.gso), _d(b.first), _d(b.seg), out, d_off, flags=flags,
           raw=raw)
        udr = torch.zeros(b.nf, dtype=torch.int16, device="cuda")
        mask = rx(out, d_off, udp_raw=udr)
        assert np.array_equal(host(mask).view(np.uint64), full), flags
        if flags == 0:
            assert (u16(udr) == 0xFFFF).all()
        else:
            assert np.array_equal(u16(udr), u16(raw)) and not (u16(udr) == 0xFFFF).all()
        assert not host(tcp_rx(out, d_off)).any()
    c = _tx.Case(rng, ipver, 4 * rng.integers(0, 400, 200))
    off = c.packed()
    tout = torch.zeros(int(off[-1]), dtype=torch.uint8, device="cuda")
    tfn = nsx.tx_ipv4_tcp_build_dev if ipver == 4 else nsx.tx_ipv6_tcp_build_dev
    tfn({k: _d(v.reshape(-1)) for k, v in c.ip.items()}, {k: _d(v) for k, v in c.fields.items()}, _d(c.data),
        _d(c.data_off), tout, _d(off))
    assert host(tcp_rx(tout, _d(off))).view(np.uint64).tolist() == mask_words(np.ones(200, bool)).tolist()
    assert not host(rx(tout, _d(off))).any()


# ---------------------------------------------------------------- graph capture
@pytest.mark.parametrize("ipver", [4, 6])
def test_udp_calls_capture_into_a_graph(ipver):
    """One tx call and one rx call captured with torch.cuda.graph on a side stream and replayed twice: the capture
    runs nothing, each replay gives the exact frames and mask."""
    rng = np.random.default_rng([0x0DF0, ipver])
    n = 700
    c = _udp.Case(rng, ipver, 4 * rng.integers(0, 500, n))
    off = c.packed()
    want, wraw = _udp.expected(c, off, fill=FILL)
    fr, _ = _udp.frames(c)
    wv, wipr, wudr = _udp.rx_expected(ipver, *_udp.concat(fr))
    assert wv.all()
    ip, ports = _soa(c)
    data, d_doff, d_off = _d(c.data), _d(c.data_off), _d(off)
    out = torch.full((int(off[-1]),), FILL, dtype=torch.uint8, device="cuda")
    raw = torch.zeros(n, dtype=torch.int16, device="cuda")
    mask = torch.zeros((n + 63) // 64, dtype=torch.int64, device="cuda")
    udr = torch.zeros(n, dtype=torch.int16, device="cuda")
    tx = nsx.udp_tx_ipv4_build_dev if ipver == 4 else nsx.udp_tx_ipv6_build_dev
    rx = nsx.udp_rx_ipv4_verify_dev if ipver == 4 else nsx.udp_rx_ipv6_verify_dev
    scratch = torch.empty_like(out)
    tx(ip, ports, data, d_doff, scratch, d_off)  # a first call outside capture (library and device-info setup)
    rx(scratch, d_off, mask=torch.empty_like(mask))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        tx(ip, ports, data, d_doff, out, d_off, raw=raw)
        rx(out, d_off, mask=mask, udp_raw=udr)
    torch.cuda.synchronize()
    assert (host(out) == FILL).all() and not host(mask).any()  # capture ran nothing
    for _ in range(2):
        g.replay()
        _same(off, host(out), u16(raw), want, wraw, "replay")
        assert np.array_equal(host(mask).view(np.uint64), mask_words(wv)) and np.array_equal(u16(udr), wudr)
        out.fill_(FILL)
        mask.zero_()
        torch.cuda.synchronize()


# ---------------------------------------------------------------- far offsets
@pytest.fixture(scope="module")
def arena():
    setup_gpu()
    a = torch.zeros(_far.ARENA, dtype=torch.uint8, device="cuda")
    yield a
    del a
    torch.cuda.empty_cache()


def _all_equal(t, byte):
    """One device reduction: every byte of the uint8 tensor t is `byte` (8 bytes at a time over the aligned middle)."""
    n = t.numel()
    a = min((-t.data_ptr()) % 8, n)
    m = (n - a) // 8
    word = int.from_bytes(bytes([byte]) * 8, "little", signed=True)
    ok = bool((t[:a] == byte).all()) and bool((t[a + 8 * m:] == byte).all())
    return ok and (m == 0 or bool((t[a:a + 8 * m].view(torch.int64) == word).all()))


def _check_arena(arena, pieces, what=""):
    """The arena holds exactly `pieces` (device address, bytes): each window compared on the host, the slices between
    the windows still zero by a device reduction."""
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


def _slot_lens(rng, flen):
    s = (np.asarray(flen, np.uint64) + np.uint64(3)) & ~np.uint64(3)
    s[::5] += (rng.integers(1, 17, s[::5].size) * 4).astype(np.uint64)
    return s


def _put(arena, pieces):
    arena.zero_()
    for d, b in pieces:
        if len(b):
            arena[d:d + len(b)].copy_(torch.from_numpy(np.frombuffer(bytes(b), np.uint8).copy()))


GIANT = _far.TWO32 + 100
DATA_AT = 1 << 20


@pytest.mark.parametrize("ipver", [4, 6])
def test_far_udp_tx_slots_and_payloads_past_2_32(arena, ipver):
    """d_out_off up to and past 2^32 (200 frames near 0, 400 from 2^32 - 700 upward, one across byte 2^32) and
    d_data_off past 2^32: d_data is the arena itself, frame 100's payload is 2^32 + 100 bytes — by its low word a
    100-byte frame — and is not built (nothing written, raw 0); the frames behind it take their payloads from above
    2^32. Against the model on the compact twin."""
    rng = np.random.default_rng([0x0FB3, ipver])
    n, g = _far.BUILD_NEAR + _far.BUILD_FAR, 100
    lens = rng.integers(0, 401, n)
    lens[g] = 0  # in the twin; GIANT on the device
    c = _udp.Case(rng, ipver, lens, lead=int(rng.integers(4)))
    start, twin = _far.build_slots(_slot_lens(rng, c.flen))
    want, wraw = _udp.expected(c, twin, fill=0)
    want[int(twin[g]):int(twin[g + 1])] = 0
    wraw[g] = 0
    cut = int(c.data_off[g])
    data_off = c.data_off + np.uint64(DATA_AT)
    data_off[g + 1:] += np.uint64(GIANT)
    assert int(data_off[g + 1] - data_off[g]) == GIANT and int(data_off[-1]) + 8 <= _far.ARENA
    payloads = [(DATA_AT, c.data[:cut]), (DATA_AT + cut + GIANT, c.data[cut:])]
    far_t = int(twin[_far.BUILD_NEAR])
    out = [(0, want[:far_t]), (int(start[_far.BUILD_NEAR]), want[far_t:])]
    assert out[0][0] + len(out[0][1]) + _far.GUARD <= DATA_AT - _far.GUARD
    assert out[1][0] + len(out[1][1]) + _far.GUARD <= payloads[1][0] - _far.GUARD
    _put(arena, payloads)
    raw = torch.full((n,), 0x5A5A, dtype=torch.int16, device="cuda")
    ip, ports = _soa(c)
    fn = nsx.udp_tx_ipv4_build_dev if ipver == 4 else nsx.udp_tx_ipv6_build_dev
    fn(ip, ports, arena, _d(data_off), arena, _d(start), raw=raw)
    got = u16(raw)
    assert got[g] == 0, f"the 2^32 + 100 byte payload was built: raw {got[g]:#x}"
    assert np.array_equal(got, wraw)
    _check_arena(arena, payloads + out, "udp tx")


@pytest.mark.parametrize("ipver", [4, 6])
def test_far_udp_uso_slots(arena, ipver):
    """The frames of 60 super-datagrams, the first third near 0 and the others from 2^32 - 700 upward — the cut
    falls inside a super-datagram."""
    rng = np.random.default_rng([0x0FB4, ipver])
    b = _udp.Batch(rng, ipver, rng.integers(0, 20 * 64, 60), 64, lead=int(rng.integers(4)))
    c = _udp.expand(b)
    n_near = next(f for f in range(b.nf // 3, b.nf) if b.seg[f - 1] == b.seg[f])
    start, twin = _far.build_slots(_slot_lens(rng, c.flen), n_near)
    want, wraw, _ = _udp.uso_expected(b, off=twin, fill=0)
    arena.zero_()
    ip, ports = _soa(b.sup)
    raw = torch.full((b.nf,), 0x5A5A, dtype=torch.int16, device="cuda")
    fn = nsx.udp_uso_ipv4_build_dev if ipver == 4 else nsx.udp_uso_ipv6_build_dev
    fn(ip, ports, _d(b.sup.data), _d(b.sup.data_off), _d(b.gso), _d(b.first), _d(b.seg), arena, _d(start), raw=raw)
    assert np.array_equal(u16(raw), wraw)
    far_t = int(twin[n_near])
    _check_arena(arena, [(0, want[:far_t]), (int(start[n_near]), want[far_t:])], "udp uso")


@pytest.mark.parametrize("placement", [("straddle", 1), ("wrap_frame", 0), ("wrap_empty", 0)], ids=_far.pid)
@pytest.mark.parametrize("ipver", [4, 6])
def test_far_udp_rx_offsets(arena, ipver, placement):
    """d_offsets past 2^32: 200 frames near 0, one span of about 2^32 bytes — a frame no length field can say; with
    wrap_frame its first bytes are a valid frame and its length's low word says exactly that frame — and 600 frames
    behind it, one across byte 2^32 (straddle) or all above it. Against the model on the compact twin."""
    rng = np.random.default_rng([0x0FB5, ipver, _far.PLACEMENTS.index(placement)])
    c = _udp.Case(rng, ipver, rng.integers(0, 120, _far.N_NEAR + _far.N_FAR + 1), lead=1)
    fr, _ = _udp.frames(c)
    for i in range(3, len(fr), 11):
        fr[i] = _udp.corrupt(rng, fr[i], ipver, _udp.CORRUPTIONS[(i // 11) % len(_udp.CORRUPTIONS)])
    head = fr.pop()
    if placement[0] == "wrap_frame":
        placement = ("wrap_frame", len(head))
    near, far = [f.tobytes() for f in fr[:_far.N_NEAR]], [f.tobytes() for f in fr[_far.N_NEAR:]]
    r = _far.layout(near, head.tobytes() if placement[0] == "wrap_frame" else b"", far, placement, lead=1, rng=rng)
    wv, wipr, wudr = _udp.rx_expected(ipver, r.buf, r.offs)
    assert not wv[r.span] and wudr[r.span] == 0 and wv.sum() > 400
    _put(arena, r.pieces())
    got = _rx_run(ipver, arena, r.far_offs, tune=None)
    _rx_same(ipver, got, (wv, wipr, wudr), what=_far.pid(placement))
