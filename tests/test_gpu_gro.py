"""Receive coalescing on the GPU (nsx_gro_ipv4_tcp_dev / nsx_gro_ipv6_tcp_dev): every output array against the numpy
restatement tests/_gro.py (held to segmentation offload's expansion by tests/test_gro_abi.py), over outputs pre-filled
with a fill byte so that the untouched regions are compared too. Bit-exact throughout."""
import functools

import numpy as np
import pytest

import _gro
import _rx
import _tso
import _tx
from _gpu import dev, host, setup_gpu, torch, nsx, mask_words

pytestmark = pytest.mark.gpu

FILL = 0xAB
_NP = {"uint8": np.uint8, "int16": np.uint16, "int32": np.uint32, "int64": np.uint64}
_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
           np.dtype(np.uint64): np.int64}
F = _gro


def setup_module(module):
    setup_gpu()


def _d(a):
    a = np.ascontiguousarray(a)
    return dev(a.view(_SIGNED[a.dtype]))


def _fn(ipver):
    return nsx.gro_ipv4_tcp_dev if ipver == 4 else nsx.gro_ipv6_tcp_dev


def _sizes(n, ipver, nbytes):
    alen = 4 if ipver == 4 else 16
    return {k: (dt, max(count(n, alen, nbytes), 1)) for k, dt, count in nsx.GRO_FIELDS}


def _filled(n, ipver, nbytes):
    """Every output at its worst-case size, each byte FILL."""
    out = {}
    for k, (dt, cnt) in _sizes(n, ipver, nbytes).items():
        size = np.dtype(_NP[dt]).itemsize
        out[k] = torch.full((cnt * size,), FILL, dtype=torch.uint8, device="cuda").view(getattr(torch, dt))
    return out


def _gpu(buf, offs, valid, ipver, tune=None, d_valid=None):
    """One device call over FILL-filled outputs: dict of host arrays (unsigned views)."""
    n = offs.size - 1
    words = mask_words(F.valid_bits(valid, n).astype(np.uint8)) if d_valid is None else None
    d_valid = _d(words if words.size else np.zeros(1, np.uint64)) if d_valid is None else d_valid
    out = _filled(n, ipver, buf.size)
    res = _fn(ipver)(_d(buf), _d(offs), d_valid, out=out, tune=tune)
    assert all(res[k] is out[k] for k in out)
    return {k: host(v).view(_NP[dt]) for (k, v), (dt, _) in zip(res.items(), _sizes(n, ipver, buf.size).values())}


def _want(buf, offs, valid, ipver):
    """The oracle's outputs laid into FILL-filled arrays of the worst-case sizes."""
    n = offs.size - 1
    o = F.gro(buf, offs, valid, ipver)
    ns = o["n_super"]
    want = {}
    for k, (dt, cnt) in _sizes(n, ipver, buf.size).items():
        size = np.dtype(_NP[dt]).itemsize
        a = np.full(cnt * size, FILL, np.uint8).view(_NP[dt])
        v = np.asarray([ns], np.uint64) if k == "n_super" else np.asarray(o[k]).reshape(-1)
        a[:v.size] = v
        want[k] = a
    return want, o


def _same(got, want, what=""):
    for k in want:
        if not np.array_equal(got[k], want[k]):
            d = np.nonzero(got[k] != want[k])[0]
            raise AssertionError(f"{what} {k}: {d.size} entries differ, first at {d[0]}: got {got[k][d[:8]]}, "
                                 f"want {want[k][d[:8]]} (n_super got {got['n_super'][0]}, want {want['n_super'][0]})")


def _check(buf, offs, valid, ipver, tunes=(None,), what=""):
    want, o = _want(buf, offs, valid, ipver)
    for tune in tunes:
        _same(_gpu(buf, offs, valid, ipver, tune=tune), want, f"{what} tune={tune}")
    return o


# ---------------------------------------------------------------- cut cases
@pytest.mark.parametrize("opts", [False, True], ids=["noopt", "opts"])
@pytest.mark.parametrize("mss", F.MSS_SET + (1,))
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_cut_cases(ipver, mss, opts):
    """The frames segmentation offload cuts at every cut length, behind 0-3 lead bytes (the source alignment): odd mss
    makes the payloads of neighbouring frames meet inside a dword at every byte position; mss 3 and 1 make payloads
    shorter than a dword."""
    b = F.cut_batch(ipver, mss, opts, lead=1)
    for lead in range(4):
        buf, offs, valid = F.frames_of(b, lead=lead)
        o = _check(buf, offs, valid, ipver, what=f"lead={lead}")
        assert o["n_super"] == b.n and np.array_equal(o["frame_cnt"], np.diff(b.first))


# ---------------------------------------------------------------- one test per clause
def _flip(at, bit=0x01):
    def f(fr, tcp):
        fr[at] ^= bit
    return f


def _tcp(at, bit=0x01):
    def f(fr, tcp):
        fr[tcp + at] ^= bit
    return f


def _add16(at, delta, in_tcp=False):
    def f(fr, tcp):
        p = (tcp if in_tcp else 0) + at
        fr[p:p + 2] = ((int.from_bytes(fr[p:p + 2], "big") + delta) & 0xFFFF).to_bytes(2, "big")
    return f


def _doff5(fr, tcp):
    fr[tcp + 12] = 0x50  # the four option bytes become payload


CLAUSES4 = {"src": _flip(15), "dst": _flip(16), "ttl": _flip(8), "tos": _flip(1, 0x04), "ident_gap": _add16(4, 1),
            "df": _flip(6, 0x40)}
CLAUSES6 = {"src": _flip(8), "src_last": _flip(23), "dst": _flip(24), "dst_last": _flip(39), "hop": _flip(7),
            "class": _flip(1, 0x10), "class_hi": _flip(0, 0x01), "flow": _flip(3), "flow_hi": _flip(1, 0x08)}
CLAUSES_TCP = {"sport": _tcp(1), "dport": _tcp(2), "ack": _tcp(11), "ack_hi": _tcp(8, 0x80), "window": _tcp(15),
               "urgent": _tcp(19), "option_byte": _tcp(22), "option_last": _tcp(23, 0x80), "doff": _doff5,
               "byte12_low": _tcp(12, 0x01), "seq_gap": _tcp(7), "seq_back": _tcp(4, 0x80)}
BITS = {"fin": F.FIN, "syn": F.SYN, "rst": F.RST, "psh": F.PSH, "ack": F.ACK, "urg": F.URG, "ece": F.ECE, "cwr": F.CWR}
# a bit set (ACK: cleared) on frame 0 is on the c_{i-1} side of the pair (1, 0) only, on frame 2 on the c_i side of
# (2, 1) only, on frame 1 on both; these break the run ...
CTL_BREAKS = [(0, b) for b in ("fin", "syn", "rst", "psh", "ack", "urg", "ece")] + [(1, b) for b in BITS] + \
    [(2, b) for b in ("syn", "rst", "ack", "urg", "ece", "cwr")]
CTL_ALLOWED = [(2, "fin"), (2, "psh"), (0, "cwr")]  # ... and these are the flags a run may carry at its ends


@functools.lru_cache(maxsize=None)
def _three(ipver, pays=(700, 700, 700), opt=True):
    """A run of three frames of one connection, with a 4-byte MSS option: (frames, n_super of the run)."""
    rng = np.random.default_rng(0x700 + ipver)
    c = F.flow_case(rng, ipver, pays, opt=_tx.opt_bytes(rng, "mss") if opt else b"")
    frames = F.case_frames(c)
    buf, offs = F.pack(frames)
    return frames, F.gro(buf, offs, np.ones(len(frames), bool), ipver)["n_super"]


def _perturbed(ipver, change, which=1, **kw):
    frames, base = _three(ipver, **kw)
    frames = list(frames)
    fr = bytearray(frames[which])
    change(fr, 20 if ipver == 4 else 40)
    frames[which] = F.refix(fr, ipver)
    return frames, base


def _clause_ids():
    ids = [(4, k) for k in CLAUSES4] + [(6, k) for k in CLAUSES6]
    return ids + [(v, k) for v in (4, 6) for k in CLAUSES_TCP]


@pytest.mark.parametrize("ipver,name", _clause_ids(), ids=[f"v{v}-{k}" for v, k in _clause_ids()])
def test_gro_same_clause(ipver, name):
    """One thing changed in the middle frame of a three-frame run, checksums re-fixed: the run breaks (the oracle's
    n_super differs from the unperturbed run's 1) and the kernels agree with the oracle array for array."""
    change = {**(CLAUSES4 if ipver == 4 else CLAUSES6), **CLAUSES_TCP}[name]
    frames, base = _perturbed(ipver, change)
    assert base == 1
    buf, offs = F.pack(frames, lead=ipver % 4)
    o = _check(buf, offs, np.ones(3, bool), ipver, what=name)
    assert o["n_super"] != base


@pytest.mark.parametrize("which,bit", CTL_BREAKS + CTL_ALLOWED, ids=[f"f{w}-{b}" for w, b in CTL_BREAKS + CTL_ALLOWED])
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_control_bits(ipver, which, bit):
    """Each control bit flipped on the first, middle or last frame of a run of ACK frames: on either side of a pair.
    FIN / PSH on the last frame and CWR on the first are what a run may carry; they come out in `control`."""
    frames, base = _perturbed(ipver, _tcp(13, BITS[bit]), which=which)
    buf, offs = F.pack(frames, lead=1)
    o = _check(buf, offs, np.ones(3, bool), ipver, what=f"{which}-{bit}")
    if (which, bit) in CTL_ALLOWED:
        assert o["n_super"] == base == 1 and o["control"][0] == F.ACK | BITS[bit]
    else:
        assert o["n_super"] != base


JOIN_CASES = [(v, c) for v in (4, 6) for c in ("longer", "zero", "mask_cleared", "doff_past_end", "doff_lt5")] + \
    [(4, "ip_options")]


@pytest.mark.parametrize("ipver,case", JOIN_CASES, ids=[f"v{v}-{c}" for v, c in JOIN_CASES])
def test_gro_join_clauses_and_membership(ipver, case):
    """A longer payload and a zero payload in the middle frame; its mask bit cleared; its data offset past the end
    of the segment, and below 5, with the mask bit still set (the receive pass does not look at it); IPv4 options
    (a member, but a singleton)."""
    valid = np.ones(3, bool)
    if case in ("longer", "zero"):
        frames, base = _three(ipver)
        frames, _ = _three(ipver, pays=(700, 701 if case == "longer" else 0, 700))
    elif case == "mask_cleared":
        frames, base = _three(ipver)
        valid[1] = False
    elif case == "ip_options":
        frames, base = _three(ipver)
        fr = bytearray(frames[1])
        fr = fr[:20] + bytes([1, 1, 1, 0]) + fr[20:]
        fr[0] = 0x46
        fr[2:4] = len(fr).to_bytes(2, "big")
        frames = [frames[0], F.refix(fr, 4), frames[2]]
    else:
        # 30-byte payloads without options: a 50-byte segment, shorter than doff 15 says
        frames, base = _perturbed(ipver, lambda fr, tcp: fr.__setitem__(tcp + 12, 0xF0 if case == "doff_past_end" else 0x40),
                                  pays=(30, 30, 30), opt=False)
    assert base == 1
    buf, offs = F.pack(list(frames), lead=3)
    o = _check(buf, offs, valid, ipver, what=case)
    assert o["n_super"] != base
    if case in ("mask_cleared", "doff_past_end", "doff_lt5"):
        assert o["frame_seg"].tolist() == [0, F.NONE, 1]
    if case == "ip_options":
        assert o["frame_seg"].tolist() == [0, 1, 2] and o["opt_off"].tolist() == [0, 4, 8, 12]


def test_refixed_frames_pass_the_receive_pass():
    """The perturbed frames are valid frames: the GPU receive pass accepts all three (so the all-ones mask of the
    clause tests is the mask a caller would have)."""
    for ipver in (4, 6):
        for change in (_tcp(22), _doff5, _flip(8 if ipver == 4 else 7)):
            frames, _ = _perturbed(ipver, change)
            buf, offs = F.pack(frames, lead=2)
            rx = nsx.rx_ipv4_tcp_verify_dev if ipver == 4 else nsx.rx_ipv6_tcp_verify_dev
            assert int(host(rx(_d(buf), _d(offs))).view(np.uint64)[0]) == 0b111


# ---------------------------------------------------------------- the window rule
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_window_rule(ipver):
    """1000, 800, 600, 400, 200 gives [1000, 800], [600], [400], [200]; 1000, 1000, 500, 500 gives [1000, 1000, 500],
    [500]: every frame of a run but the last carries the same payload."""
    rng = np.random.default_rng(0x720 + ipver)
    for pays, cnt in (((1000, 800, 600, 400, 200), [2, 1, 1, 1]), ((1000, 1000, 500, 500), [3, 1]),
                      ((500, 1000, 1000, 1000, 1), [1, 4]), ((7, 7, 7, 7, 7, 3, 7, 7), [6, 2])):
        buf, offs = F.pack(F.case_frames(F.flow_case(rng, ipver, pays)), lead=1)
        o = _check(buf, offs, np.ones(len(pays), bool), ipver, what=str(pays))
        assert o["frame_cnt"].tolist() == cnt


# ---------------------------------------------------------------- run lengths and scan seams
@functools.lru_cache(maxsize=None)
def _runs(ipver, lengths, pay=100, tail=37, psh=True):
    """Runs of the given lengths, each its own connection, the last frame of each short; psh: every third one with
    PSH on all its frames."""
    rng = np.random.default_rng(0x740 + ipver + len(lengths))
    frames = []
    for i, L in enumerate(lengths):
        pays = [pay] * (L - 1) + [tail if L > 1 else pay]
        frames += F.case_frames(F.flow_case(rng, ipver, pays, opt=_tx.opt_bytes(rng, "mss") if i % 2 else b"",
                                            ctl=F.ACK | (F.PSH if psh and i % 3 == 0 else 0)))
    return F.pack(frames, lead=3)


@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_run_lengths_and_scan_seams(ipver):
    """Runs of 1, 2, 63, 64, 65 and 257 frames (the head pass's waves own 63 frames, the copy pass's 16): with 64
    frames per scan block the runs straddle block boundaries, with 16 every block seam falls inside a run."""
    lengths = (1, 2, 63, 64, 65, 257, 1, 1, 64)
    buf, offs = _runs(ipver, lengths)
    n = offs.size - 1
    o = _check(buf, offs, np.ones(n, bool), ipver,
               tunes=(None, dict(run_segs=64), dict(run_segs=16), dict(run_segs=100, blocks_per_cu=1)))
    # PSH on every frame of every third run: those frames stay singletons (c_{i-1} & PSH)
    assert o["frame_cnt"].tolist() == sum(([1] * L if i % 3 == 0 else [L] for i, L in enumerate(lengths)), [])
    valid = np.ones(n, bool)
    valid[[0, 70, 200, n - 1]] = False
    _check(buf, offs, valid, ipver, tunes=(None, dict(run_segs=64)), what="holes")


@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_just_above_the_default_scan_block(ipver):
    """4,100 frames of 8 payload bytes in runs of 300: two scan blocks without any tune."""
    buf, offs = _runs(ipver, (300,) * 13 + (200,), pay=8, tail=5, psh=False)
    assert offs.size - 1 == 4100
    o = _check(buf, offs, np.ones(4100, bool), ipver)
    assert o["n_super"] == 14 and o["frame_cnt"].tolist() == [300] * 13 + [200]


# ---------------------------------------------------------------- wraps
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_sequence_and_ident_wrap(ipver):
    rng = np.random.default_rng(0x760 + ipver)
    frames = F.case_frames(F.flow_case(rng, ipver, [700] * 4, seq0=(1 << 32) - 1000, ident0=0xFFFE))
    buf, offs = F.pack(frames)
    o = _check(buf, offs, np.ones(4, bool), ipver)
    assert o["n_super"] == 1 and o["seq_num"][0] == (1 << 32) - 1000 and o["frame_cnt"][0] == 4


# ---------------------------------------------------------------- mixed batches
@pytest.mark.parametrize("wire", [False, True], ids=["reference_byte12", "wire_byte12"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_mixed_batches_with_the_receive_pass_mask(ipver, wire):
    """tests/_rx.py batches, valid and broken in every way the receive pass distinguishes, with the mask from the GPU
    receive pass itself. As the reference serialises them (byte 12 = the word count itself, data offset 0 to a
    receiver) every frame is a non-member; with byte 12 in wire form the valid ones are members."""
    rng = np.random.default_rng(0x780 + ipver + wire)
    kinds = _rx.KINDS if ipver == 4 else _rx.KINDS6
    buf, offs, ks = _rx.batch(rng, 300, kinds, lead=int(rng.integers(4)), max_payload=300, ip=ipver)
    if wire:
        for i in range(300):
            a, e = int(offs[i]), int(offs[i + 1])
            fr = bytearray(buf[a:e].tobytes())
            iph = 40 if ipver == 6 else (fr[0] & 15) * 4 if fr else 0
            if iph >= 20 and len(fr) >= iph + 20 and fr[0] >> 4 == ipver:
                fr[iph + 12] = (fr[iph + 12] << 4) & 0xFF
                if ks[i] not in ("bad_tcp_sum", "bad_ip_sum", "bad_addr"):
                    fr = F.refix(fr, ipver)
                buf[a:e] = np.frombuffer(bytes(fr), np.uint8)
    rx = nsx.rx_ipv4_tcp_verify_dev if ipver == 4 else nsx.rx_ipv6_tcp_verify_dev
    d_mask = rx(_d(buf), _d(offs))
    valid = host(d_mask).view(np.uint64)
    want, o = _want(buf, offs, valid, ipver)
    _same(_gpu(buf, offs, valid, ipver, d_valid=d_mask), want)
    if wire:
        assert 20 < o["n_super"] < 300
    else:
        assert o["n_super"] == 0 and F.valid_bits(valid, 300).sum() > 20


def test_gro_empty_batch():
    """n == 0 writes n_super = 0 and the two leading offsets, nothing else."""
    for ipver in (4, 6):
        buf, offs = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
        want, _ = _want(buf, offs, np.zeros(0, bool), ipver)
        assert want["n_super"][0] == 0 and want["opt_off"][0] == 0 and want["data_off"][0] == 0
        _same(_gpu(buf, offs, np.zeros(0, bool), ipver), want)


# ---------------------------------------------------------------- the loop on the device
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_closes_the_loop_on_the_device(ipver):
    """tso_build → rx_verify → gro → tso_build without leaving the device: 4-multiple frame lengths, so the build's
    out_off is the receive pass's offsets; the second buffer equals the first byte for byte."""
    rng = np.random.default_rng(0x7A0 + ipver)
    n = 60
    mss = np.array([(1460, 1448, 536, 8)[i % 4] for i in range(n)], np.uint32)
    lens = 4 * rng.integers(0, 2 * mss)
    keys = ["mss", "nop_nop", "k2len40"]  # nop_nop: 2 option bytes + 2 bytes of padding, carried as 4 option bytes
    ob = [_tx.opt_bytes(rng, keys[i % 3]) if i % 3 else b"" for i in range(n)]
    b = _tso.Batch(rng, ipver, lens, mss, opts=ob)
    b.sup.fields["control"][:] = np.resize(np.array([0x10, 0x18, 0x19, 0x90, 0xD9], np.uint8), n)
    F.wire_offset(b.sup)
    c = _tso.expand(b)
    assert not (c.flen % 4).any() and b.nf > 2 * n
    s = b.sup
    tso = nsx.tso_ipv4_tcp_build_dev if ipver == 4 else nsx.tso_ipv6_tcp_build_dev
    d_off = _d(b.off)
    first = torch.full((int(b.off[-1]),), FILL, dtype=torch.uint8, device="cuda")
    tso({k: _d(v.reshape(-1)) for k, v in s.ip.items()}, {k: _d(v) for k, v in s.fields.items()}, _d(s.data),
        _d(s.data_off), _d(b.mss), _d(b.first), _d(b.seg), first, d_off, opts=_d(s.opts), opt_off=_d(s.opt_off))
    rx = nsx.rx_ipv4_tcp_verify_dev if ipver == 4 else nsx.rx_ipv6_tcp_verify_dev
    mask = rx(first, d_off)
    g = _fn(ipver)(first, d_off, mask)
    ns = int(g["n_super"].item())
    assert ns == n
    frame_first = torch.zeros(ns + 1, dtype=torch.int64, device="cuda")
    frame_first[1:] = torch.cumsum(g["frame_cnt"][:ns].to(torch.int64), 0)
    assert int(frame_first[-1].item()) == b.nf
    second = torch.full((int(b.off[-1]),), FILL, dtype=torch.uint8, device="cuda")
    tso({k: g[k][:ns * (1 if k not in ("src", "dst") else (4 if ipver == 4 else 16))] for k in nsx.IP_FIELDS},
        {k: g[k][:ns] for k, _ in nsx.BUILD_FIELDS}, g["data"], g["data_off"][:ns + 1], g["mss"][:ns], frame_first,
        g["frame_seg"], second, d_off, opts=g["opts"], opt_off=g["opt_off"][:ns + 1])
    a, z = host(first), host(second)
    assert np.array_equal(a, z), np.nonzero(a != z)[0][:8]
    assert np.array_equal(a, _tso.expected(b, fill=FILL)[0])
