"""The ICMP receive verify on the GPU (nsx_icmp_rx_ipv4_verify_dev / nsx_icmp_rx_ipv6_verify_dev): the mask words, both
raw sums and the type words — each with a guard entry over a fill byte — bit-exact against the numpy restatement
tests/_icmp.py, over every launch shape nsx_icmp_tune.h offers."""
import numpy as np
import pytest

import _far
import _icmp as M
import _icmp_gen as G
import _icmp_gpu as GPU
from _gpu import host, setup_gpu, torch, nsx
from _icmp_gpu import arena  # noqa: F401  (the module's 4 GiB fixture)

pytestmark = pytest.mark.gpu
d = GPU.d
TUNES = (None, dict(blocks_per_cu=1, run_segs=1), dict(blocks_per_cu=1, run_segs=7), dict(blocks_per_cu=2, run_segs=64))
LANE_MAX = 256  # ICMP bytes up to which a lane sums its own message (csrc/icmp_kernels.hip kLaneMax)


def setup_module(module):
    setup_gpu()


def _rng(*key):
    return np.random.default_rng([0x1CE1, *key])


def _echo(rng, ipver, data_len, options=b""):
    data = rng.integers(0, 256, data_len, dtype=np.uint8).tobytes()
    kw = dict(options=options) if ipver == 4 else {}
    return G.icmp_frame(rng, ipver, 8 if ipver == 4 else 128, 0, data, **kw)


@pytest.mark.parametrize("ipver", [4, 6])
def test_each_malformation_on_its_own(ipver):
    """One valid frame and one frame of every invalid kind, each kind three times over (the lengths and alignments
    differ), every launch shape: the verdicts, raws and type words are the model's."""
    rng = _rng(1, ipver)
    kinds = [k for k in G.RX_KINDS[ipver] for _ in range(3)]
    fr = [G.rx_frame(rng, k, ipver, max_pay=int(rng.choice([20, 400]))) for k in kinds]
    for lead in (0, 3):
        buf, offs = M.pack(fr, lead=lead)
        v = GPU.rx_check(buf, offs, ipver, tunes=TUNES, what=f"malformations lead {lead}")
        assert v["ok"].tolist() == [k == "valid" for k in kinds]
        assert (v["type"][~v["ok"]] == 0xFFFF).all() and (v["type"][v["ok"]] != 0xFFFF).all()


def test_ipv4_options_and_minimal_frames():
    """IHL 5, 6 and 15 with messages of 8 bytes (the least), 9 and 200; a header checksum that is wrong only inside the
    options; the 8-byte message one byte short."""
    rng = _rng(2)
    fr = []
    for ihl in (5, 6, 15):
        opt = rng.integers(0, 256, 4 * (ihl - 5), dtype=np.uint8).tobytes()
        fr += [_echo(rng, 4, L, opt) for L in (0, 1, 192)]
        if ihl > 5:
            g = bytearray(_echo(rng, 4, 4, opt))
            g[4 * ihl - 1] ^= 0x10
            fr.append(bytes(g))
        fr.append(M.ip4(1, GPU.B4, GPU.A4, M.icmp4(8, 0, bytes(4))[:7], options=opt))
    for lead in range(4):
        buf, offs = M.pack(fr, lead=lead)
        v = GPU.rx_check(buf, offs, 4, tunes=(None, dict(run_segs=3)), what=f"options lead {lead}")
        assert v["ok"].sum() == 9 and (v["ip_raw"] != 0).all()


@pytest.mark.parametrize("ipver", [4, 6])
def test_the_lane_and_wave_split_and_the_longest_frames(ipver):
    """Messages of 255, 256, 257 and 258 ICMP bytes — either side of the length up to which a lane sums its own —
    1 KiB rows' edges, and the longest frame an IP length field can say (65,535 bytes; IPv6: a 65,535-byte payload),
    valid and with its last byte wrong, at every alignment."""
    rng = _rng(3, ipver)
    lens = [LANE_MAX - 9, LANE_MAX - 8, LANE_MAX - 7, LANE_MAX - 6, 1016, 1017, 2040, 2041, 2048 + 1015]
    fr = [_echo(rng, ipver, L) for L in lens]
    top = 65535 - 20 - 8 if ipver == 4 else 65535 - 8
    big = _echo(rng, ipver, top)
    assert len(big) == (65535 if ipver == 4 else 65575)
    fr += [big, big[:-1] + bytes([big[-1] ^ 1])]
    for lead in range(4):
        buf, offs = M.pack(fr, lead=lead)
        v = GPU.rx_check(buf, offs, ipver, tunes=(None, dict(blocks_per_cu=1, run_segs=2)), what=f"split lead {lead}")
        assert v["ok"].tolist() == [True] * (len(lens) + 1) + [False]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 128, 129, 1000])
@pytest.mark.parametrize("ipver", [4, 6])
def test_mask_words_across_64_and_65_frames(ipver, n):
    """Bits past n in the last word are 0, no word past ceil(n/64) is written (n == 0 writes none), the entries behind
    the n-th of every array stay."""
    buf, offs, kinds = G.rx_batch(n, ipver, n=max(n, 2 * len(G.RX_KINDS[ipver])))
    offs = offs[:n + 1]
    v = GPU.rx_check(buf, offs, ipver, tunes=TUNES[:2] + TUNES[3:], what=f"n {n}")
    assert n < 63 or 0 < v["ok"].sum() < n


@pytest.mark.parametrize("ipver", [4, 6])
def test_nullable_outputs(ipver):
    """Every raw / type output may be NULL: the mask is the same."""
    buf, offs, _ = G.rx_batch(100, ipver)
    n = offs.size - 1
    w, v = GPU.rx_want(buf, offs, ipver)
    fn = nsx.icmp_rx_ipv4_verify_dev if ipver == 4 else nsx.icmp_rx_ipv6_verify_dev
    mask = fn(d(buf), d(offs))
    assert np.array_equal(GPU.bits_of(mask, n), v["ok"])
    typ = GPU.filled(n + 1, torch.int16)
    mask = fn(d(buf), d(offs), type=typ, tune=dict(run_segs=64))
    assert np.array_equal(GPU.bits_of(mask, n), v["ok"]) and np.array_equal(host(typ).view(np.uint16), w["type"])


@pytest.mark.parametrize("ipver", [4, 6])
def test_graph_capture_and_replay(ipver):
    """The call captured into a torch.cuda.graph runs nothing at capture and gives the model's outputs on replay."""
    buf, offs, _ = G.rx_batch(101, ipver)
    n = offs.size - 1
    w, v = GPU.rx_want(buf, offs, ipver)
    fn = nsx.icmp_rx_ipv4_verify_dev if ipver == 4 else nsx.icmp_rx_ipv6_verify_dev
    d_buf, d_offs = d(buf), d(offs)
    mask = GPU.filled((n + 63) // 64 + 1, torch.int64)
    raw, typ = GPU.filled(n + 1, torch.int16), GPU.filled(n + 1, torch.int16)
    fn(d_buf, d_offs)  # a first call outside capture (library and device-info setup)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn(d_buf, d_offs, mask=mask, icmp_raw=raw, type=typ)
    torch.cuda.synchronize()
    assert (host(mask).view(np.uint8) == GPU.FILL).all() and (host(typ).view(np.uint8) == GPU.FILL).all()
    g.replay()
    assert np.array_equal(host(mask).view(np.uint64), w["mask"])
    assert np.array_equal(host(raw).view(np.uint16), w["icmp_raw"]) and np.array_equal(host(typ).view(np.uint16), w["type"])


@pytest.mark.parametrize("placement", [("straddle", 1), ("wrap_frame", 0)], ids=_far.pid)
@pytest.mark.parametrize("ipver", [4, 6])
def test_frames_past_two_to_the_32(arena, ipver, placement):  # noqa: F811
    """A batch whose offsets pass 2^32 (tests/_far.layout): the far frames, one of them across byte 2^32, get the
    verdicts of the compact twin; a span of 2^32 + len(f) bytes that starts with a valid message f does not verify (a
    kernel keeping only the low word of its length would accept it); nothing in 4 GiB is written."""
    rng = _rng(4, ipver, _far.PLACEMENTS.index(placement))
    near = [G.rx_frame(rng, str(rng.choice(G.RX_KINDS[ipver])), ipver, 100) for _ in range(150)]
    far = [G.rx_frame(rng, str(rng.choice(G.RX_KINDS[ipver], p=G._weights(len(G.RX_KINDS[ipver])))), ipver, 1400)
           for _ in range(400)]
    f = _echo(rng, ipver, 80)
    head = f + rng.integers(0, 256, _far.HEAD - len(f), dtype=np.uint8).tobytes()
    if placement[0] == "wrap_frame":
        placement = ("wrap_frame", len(f))
    r = _far.layout(near, head, far, placement, lead=int(rng.integers(4)), rng=rng)
    w, v = GPU.rx_want(r.buf, r.offs, ipver)
    assert not v["ok"][r.span] and v["ok"][r.span + 1:].sum() > 100
    if placement[0] == "wrap_frame":
        assert M.verify_frame(f, ipver)[0]
    GPU.put(arena, r.pieces())
    got = GPU.rx_gpu(r.buf, r.offs, ipver, d_buf=arena, d_offs=d(r.far_offs))
    for k in ("mask", "ip_raw", "icmp_raw", "type"):
        assert np.array_equal(got[k], w[k]), k
    GPU.check_arena(arena, r.pieces(), "rx")
