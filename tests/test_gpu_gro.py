"""Receive coalescing on the GPU (nsx_gro_ipv4_tcp_dev / nsx_gro_ipv6_tcp_dev): every output array against the numpy
restatement tests/_gro.py (held to segmentation offload's expansion by tests/test_gro_abi.py), over outputs pre-filled
with a fill byte so that the untouched regions are compared too. Bit-exact throughout."""
import functools

import numpy as np
import pytest

import _gro
import _gro_gpu as G
import _rx
import _tso
import _tx
from _gpu import host, setup_gpu, torch, nsx

pytestmark = pytest.mark.gpu

F = _gro
FILL = G.FILL
_d, _fn, _filled, _want, _same, _check = G.d, G.fn, G.filled, G.want, G.same, G.check


def setup_module(module):
    setup_gpu()


def _gpu(buf, offs, valid, ipver, tune=None, d_valid=None):
    return G.gpu(buf, offs, valid, ipver, tune=tune, d_mask=d_valid)


# ---------------------------------------------------------------- cut cases
@pytest.mark.parametrize("opts", [False, True], ids=["noopt", "opts"])
@pytest.mark.parametrize("mss", F.MSS_SET + (1, 8960))
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_cut_cases(ipver, mss, opts):
    """The frames segmentation offload cuts at every cut length, behind 0-3 lead bytes (the source alignment): odd mss
    makes the payloads of neighbouring frames meet inside a dword at every byte position; mss 3 and 1 make payloads
    shorter than a dword; mss 8960 (jumbo frames) makes every full payload five row pairs of the copy."""
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


# ---------------------------------------------------------------- the copy's row pairs
ROW_PAIR_P = (2032, 2047, 2048, 2049, 2064, 4095, 4096, 4097, 8960)


@functools.lru_cache(maxsize=None)
def _row_pair_frames(ipver, opt, P, k):
    """A one-frame connection with k payload bytes, then a second connection: three frames of P and a 5-byte tail."""
    rng = np.random.default_rng(0x7B0 + 64 * P + 4 * k + ipver + opt)
    ob = _tx.opt_bytes(rng, "mss") if opt else b""
    return tuple(F.case_frames(F.flow_case(rng, ipver, [k], opt=ob)) +
                 F.case_frames(F.flow_case(rng, ipver, [P, P, P, 5], opt=ob)))


@pytest.mark.parametrize("P", ROW_PAIR_P)
@pytest.mark.parametrize("opt", [False, True], ids=["noopt", "opt"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_row_pair_boundary(ipver, opt, P):
    """The copy takes a payload in row pairs of 2 x 64 chunks of 16 bytes; a payload of more than 128 chunks goes
    round the pair loop again (c0 > 0). The second super-segment's destination starts k bytes into a 16-byte chunk
    (k = 0..15, the payload of the one-frame connection before it) and its source 0-3 lead bytes off, so the chunk
    count ceil((k + P) / 16) crosses 128 (P around 2048), 256 (around 4096) and 560 (8960) at every destination and
    source alignment; the frames after the first of the run start at k + P and k + 2P. Against the model, and through
    segmentation offload on the device: every frame comes back."""
    chunks = {(k + P + 15) // 16 for k in range(16)}
    if P in (2047, 2048, 4095, 4096, 8960):
        assert chunks == {(P + 15) // 16, (P + 15) // 16 + 1} and min(chunks) in (128, 256, 560)
    for k in range(16):
        frames = list(_row_pair_frames(ipver, opt, P, k))
        for lead in range(4):
            buf, offs = F.pack(frames, lead=lead)
            valid = np.ones(5, bool)
            o = _check(buf, offs, valid, ipver, what=f"k={k} lead={lead}")
            assert o["frame_cnt"].tolist() == [1, 4] and o["data_off"].tolist() == [0, k, k + 3 * P + 5]
            ps = G.assert_round_trip(buf, offs, valid, ipver, what=f"k={k} lead={lead}")
            assert ps.tolist() == [0, 1, 2, 3, 4]


# ---------------------------------------------------------------- maximal frames
def _maximal_batch(ipver, opt):
    """Three frames as long as the IP length field allows and a 9-byte tail (one connection), a frame with a valid
    header and 200,000 bytes in all, for IPv6 a maximal frame with one byte appended (one more than its payload length
    field can say), and a second connection of two small frames: (buf, offsets, the maximal payload)."""
    rng = np.random.default_rng(0x7B8 + ipver + opt)
    ob = _tx.opt_bytes(rng, "nop_nop_k2len10") if opt else b""
    assert len(ob) == (12 if opt else 0)
    top = _tx.WIRE_MAX[ipver] - 20 - len(ob)
    frames = F.case_frames(F.flow_case(rng, ipver, [top, top, top, 9], opt=ob))
    assert len(frames[0]) == (65535 if ipver == 4 else 65575)
    long = frames[0] + rng.integers(0, 256, 200_000 - len(frames[0]), dtype=np.uint8).tobytes()
    extra = [frames[2] + b"\x00"] if ipver == 6 else []
    frames = frames + [long] + extra + F.case_frames(F.flow_case(rng, ipver, [100, 100]))
    return F.pack(frames, lead=1 + opt) + (top,)


@pytest.mark.parametrize("opt", [False, True], ids=["noopt", "opt12"])
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_maximal_frames(ipver, opt):
    """IPv4 total length 65535 (payload 65495, 65483 behind 12 option bytes) and IPv6 payload length 65535 (a
    65,575-byte frame): three of them and a tail are one super-segment whose mss is that payload, and segmentation
    offload, its length limit exactly met, gives the frames back. A 200,000-byte frame and an IPv6 frame one byte
    longer than its length field says are non-members although their valid bits are set."""
    buf, offs, top = _maximal_batch(ipver, opt)
    n = offs.size - 1
    valid = np.ones(n, bool)
    o = _check(buf, offs, valid, ipver, tunes=(None, dict(run_segs=16, blocks_per_cu=1)))
    assert o["frame_cnt"].tolist() == [4, 2] and o["mss"].tolist() == [top, 100]
    assert top == {(4, False): 65495, (4, True): 65483, (6, False): 65515, (6, True): 65503}[ipver, opt]
    assert o["frame_seg"].tolist() == [0] * 4 + [F.NONE] * (n - 6) + [1, 1]
    ps = G.assert_round_trip(buf, offs, valid, ipver)
    assert ps.tolist() == [0, 1, 2, 3, n - 2, n - 1]
    # keyed by flow: the same super-segments (in key order), the non-members last
    g = _check(buf, offs, valid, ipver, flow=True)
    assert sorted(g["frame_cnt"].tolist()) == [2, 4] and sorted(g["order"][:6].tolist()) == [0, 1, 2, 3, n - 2, n - 1]
    assert sorted(G.assert_round_trip(buf, offs, valid, ipver, flow=True).tolist()) == [0, 1, 2, 3, n - 2, n - 1]


# ---------------------------------------------------------------- the emit grid's second trip
@pytest.mark.parametrize("ipver", [4, 6])
def test_gro_emit_grid_takes_a_second_trip(ipver):
    """The emit pass's grid is min(groups / 4, CUs x blocks_per_cu) workgroups of four 16-frame wave tasks: at
    blocks_per_cu = 1, 64 x CUs + 21 frames send the first workgroups round the grid-stride loop again, the last of
    them with a 5-frame group. Four connections delivered one after the other, every seventh frame a short tail that
    ends a run, every 997th valid bit clear."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * cus + 21
    assert n > 64 * cus and (n + 15) // 16 > 4 * cus
    buf, offs = F.pack([f for c in F.cycle_connections(ipver, n) for f in c], lead=ipver % 4)
    assert offs.size - 1 == n
    valid = np.ones(n, bool)
    valid[996::997] = False
    o = _check(buf, offs, valid, ipver, tunes=(dict(blocks_per_cu=1),))
    assert n // 7 <= o["n_super"] <= n // 7 + 4 + 2 * (n // 997 + 1) and o["frame_cnt"].max() == 7


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
