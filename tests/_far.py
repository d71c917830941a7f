"""Far layouts: batches whose offsets pass 2^32 and which hold one frame of about 2^32 bytes, with every expected value
taken from a compact twin. Shared by tests/test_far_layout.py (no GPU) and tests/test_gpu_far_offsets.py.

Every device entry point takes 64-bit byte offsets and every kernel narrows them to 32 bits behind an invariant written
next to the narrowing (include/nsx_csum.h takes "n+1 non-decreasing entries"). A far batch is three runs of frames over
one offsets array: `near` (about 200 frames behind 0-3 lead bytes), `span` (one frame of S bytes) and `far` (about 600
frames, 40-120 B or 40-1500 B). Three placements of S:

  straddle a   the span ends at 2^32 - 700 + a, a in 0..3: one far frame lies across byte 2^32, every later one starts
               above it, at every alignment over the four a;
  wrap_frame   S = 2^32 + len(f): the span's first len(f) bytes are a frame f that the pass would accept if the span
               were that short (its low word says so);
  wrap_empty   S = 2^32: the low word says 0.

Only the first HEAD bytes of the span are defined (plus, for the checksum passes, a few 16-bit markers); the rest is
zero. The compact twin holds the same frames with the span shortened by D, a multiple of 2^17, to 2^17 + S mod 2^17
bytes: the head, the span's low 17 length bits and every far frame's address modulo 2^17 (so modulo 128) are kept, and
the span stays longer than any length field can say. The project's models run on the twin unchanged; outputs that
carry an absolute offset are D larger behind the span on the device. The low-32 twin is what a kernel keeping only the
low word of the span's length would see: the span S mod 2^32 bytes long. The 4 GiB arena is never made on the host:
`ranges` says which device bytes come from which twin bytes.

No torch and no GPU at import."""
import numpy as np

import _gro
import _gro_flow
import _nat
import _parse
import _rx
from oracle import csum_oracle as O

TWO32 = 1 << 32
GRAIN = 1 << 17
HEAD = 256                      # defined bytes at the start of the span
ARENA = TWO32 + (8 << 20)       # device bytes every far batch fits in
GUARD = 64
N_NEAR, N_FAR = 200, 600
STRADDLE_BACK = 700             # the span of a straddle placement ends this far (less a) before byte 2^32
PLACEMENTS = (("straddle", 0), ("straddle", 1), ("straddle", 2), ("straddle", 3), ("wrap_frame", 0), ("wrap_empty", 0))
WRAPS = (("wrap_frame", 0), ("wrap_empty", 0))
MIXES = ("small", "large")      # far frames of 40-120 B (whole LDS-form runs) and of 40-1500 B (streamed runs)


def pid(p):
    return p[0] + (str(p[1]) if p[0] == "straddle" else "")


class Far:
    """buf, offs: the compact twin (offs uint64[n+1]); far_offs: the device offsets; span: the span's frame index; S,
    S_twin, D = S - S_twin; ranges: three (device start, twin start, length) triples — near (with the lead bytes), the
    span's head, far (with the tail bytes); marks: (device address, twin address, bytes) markers inside the span;
    low_buf, low_offs: the low-32 twin (wrap placements only)."""

    def pieces(self, twin_buf=None):
        """(device address, bytes) of everything defined in the arena when the twin holds twin_buf (default: the
        batch as built): the three ranges and the markers."""
        twin_buf = self.buf if twin_buf is None else twin_buf
        return [(d, twin_buf[t:t + n]) for d, t, n in self.ranges] + \
            [(d, twin_buf[t:t + len(b)]) for d, t, b in self.marks]


def windows(pieces):
    """Sorted, merged (start, end) device byte windows: every piece with GUARD bytes on either side."""
    out = []
    for lo, hi in sorted((max(0, d - GUARD), min(ARENA, d + len(b) + GUARD)) for d, b in pieces):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def window_bytes(pieces, lo, hi):
    """What device bytes [lo, hi) must hold: the pieces' bytes, zero everywhere else."""
    out = np.zeros(hi - lo, np.uint8)
    for d, b in pieces:
        a, z = max(d, lo), min(d + len(b), hi)
        if z > a:
            out[a - lo:z - lo] = np.frombuffer(bytes(b[a - d:z - d]), np.uint8)
    return out


def layout(near, head, far, placement, lead=0, tail=3, marks=(), rng=None):
    """near, far: lists of frames (bytes); head: at most HEAD bytes, the span's defined start (for wrap_frame it begins
    with the frame f and `placement` is ("wrap_frame", len(f))); marks: (position relative to the span's start, bytes)
    inside the undefined part of the span, device side. Lead and tail bytes are junk from rng (zeros without one)."""
    kind, arg = placement
    assert len(head) <= HEAD
    junk = (lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()) if rng is not None else (lambda k: bytes(k))
    lead_b, tail_b = junk(lead), junk(tail)
    near_len = sum(len(f) for f in near)
    s0 = lead + near_len
    if kind == "straddle":
        S = TWO32 - STRADDLE_BACK + arg - s0
    elif kind == "wrap_frame":
        assert 0 < arg <= len(head)
        S = TWO32 + arg
    else:
        assert kind == "wrap_empty"
        S = TWO32
    S_twin = GRAIN + S % GRAIN
    D = S - S_twin
    assert D % GRAIN == 0 and GRAIN <= S_twin < 2 * GRAIN
    far_b = b"".join(far)
    span = np.zeros(S_twin, np.uint8)
    span[:len(head)] = np.frombuffer(bytes(head), np.uint8)
    r = Far()
    r.marks = []
    for k, (rel, b) in enumerate(marks):
        assert HEAD <= rel and rel + len(b) <= S
        # the twin's marker D bytes earlier where that is inside the twin's span; else at a free address of the same
        # parity (the Internet checksum of a span sees a 16-bit value and the parity of its address, nothing more)
        t = rel - D
        if not (HEAD <= t and t + len(b) <= S_twin):
            t = HEAD + 64 * (k + 1) + (rel & 1)
        assert not span[t:t + len(b)].any(), "markers overlap in the twin"
        span[t:t + len(b)] = np.frombuffer(bytes(b), np.uint8)
        r.marks.append((s0 + rel, s0 + t, bytes(b)))
    r.buf = np.concatenate([np.frombuffer(lead_b + b"".join(near), np.uint8), span,
                            np.frombuffer(far_b + tail_b, np.uint8)])
    lens = [len(f) for f in near] + [S_twin] + [len(f) for f in far]
    r.offs = np.zeros(len(lens) + 1, np.uint64)
    r.offs[1:] = np.cumsum(lens)
    r.offs += np.uint64(lead)
    r.span, r.S, r.S_twin, r.D, r.n = len(near), S, S_twin, D, len(lens)
    r.far_offs = r.offs.copy()
    r.far_offs[r.span + 1:] += np.uint64(D)
    assert int(r.far_offs[-1]) + tail <= ARENA
    r.ranges = [(0, 0, s0), (s0, s0, HEAD), (s0 + S, s0 + S_twin, len(far_b) + tail)]
    r.low_buf = r.low_offs = None
    if kind != "straddle":
        S_low = S % TWO32
        r.low_buf = np.frombuffer(lead_b + b"".join(near) + bytes(head[:S_low]) + far_b + tail_b, np.uint8).copy()
        lens[r.span] = S_low
        r.low_offs = np.zeros(len(lens) + 1, np.uint64)
        r.low_offs[1:] = np.cumsum(lens)
        r.low_offs += np.uint64(lead)
    r.placement = placement
    return r


def crossing(far_offs):
    """The frames that hold byte 2^32 with bytes on both sides of it."""
    o = np.asarray(far_offs, np.uint64).astype(object)
    return [i for i in range(len(o) - 1) if o[i] < TWO32 < o[i + 1]]


def shift_behind_span(r, v):
    """An absolute-offset output of the twin as the device gives it: D added for frames behind the span, where the
    value is an offset at all (nonzero)."""
    v = np.asarray(v, np.uint64).copy()
    tail = v[r.span + 1:]
    tail[tail != 0] += np.uint64(r.D)
    return v


def _max_payload(mix, hdr):
    """Payload bound of a far frame: frames of at most 120 B or 1500 B."""
    return (120 if mix == "small" else 1500) - hdr


def _junk_head(rng, first):
    h = bytearray(rng.integers(0, 256, HEAD, dtype=np.uint8).tobytes())
    if first is not None:
        h[0] = first
    return bytes(h)


# ---------------------------------------------------------------- the receive pass
def rx_batch(ipver, placement, mix, seed=0):
    """Mixed valid / broken / malformed frames (tests/_rx.py). wrap_frame: f is a datagram that verifies. Junk heads
    start like an IP header of the pass's version, so the IPv4 header sum of the span is not 0."""
    rng = np.random.default_rng([0xFA0, ipver, PLACEMENTS.index(placement), MIXES.index(mix), seed])
    make, kinds, hdr = (_rx.frame6, _rx.KINDS6, 60) if ipver == 6 else (_rx.frame, _rx.KINDS, 80)  # 40 B of IP options
    near = [make(rng, k, _max_payload(mix, hdr)) for k in rng.choice(kinds, N_NEAR)]
    far = [make(rng, k, _max_payload(mix, hdr)) for k in rng.choice(kinds, N_FAR)]
    if placement[0] == "wrap_frame":
        f = make(rng, "valid", 100)
        head, placement = f, ("wrap_frame", len(f))
    else:
        head = _junk_head(rng, 0x60 if ipver == 6 else 0x45)
    return layout(near, head, far, placement, lead=int(rng.integers(4)), rng=rng)


def rx_model(ipver, buf, offs):
    return (O.c_rx_ipv6_tcp if ipver == 6 else O.c_rx_ipv4_tcp)(buf, offs)


# ---------------------------------------------------------------- the ragged checksum (the span is in contract)
def csum_batch(placement, mix, seed=0):
    """Segments of any bytes; the span's own sum is checked, so it carries 16-bit markers at even and odd addresses:
    around relative byte 2^31, on both sides of absolute byte 2^32 and in the last 256-byte row."""
    rng = np.random.default_rng([0xFA1, PLACEMENTS.index(placement), MIXES.index(mix), seed])
    hi = _max_payload(mix, 0)
    near = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, hi + 1, N_NEAR)]
    far = [rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in rng.integers(0, hi + 1, N_FAR)]
    head = _junk_head(rng, None)
    if placement[0] == "wrap_frame":
        placement = ("wrap_frame", 60)
    lead = int(rng.integers(4))
    probe = layout(near, head, far, placement, lead=lead)
    s0, S = int(probe.offs[probe.span]), probe.S
    rel = [(1 << 31) - 2, (1 << 31) + 1, (1 << 31) + 6]
    for a in (TWO32 - 6, TWO32 - 1, TWO32 + 4, TWO32 + 9):  # absolute addresses; -1 lies across the byte itself
        if HEAD <= a - s0 and a - s0 + 2 <= S - 300:
            rel.append(a - s0)
    rel += [S - 200, S - 101, S - 2 if placement[0] != "wrap_frame" else S - 3]
    val = [bytes([0x80 | (k + 1), 0x11 * (k + 1) & 0xFF | 1]) for k in range(len(rel))]
    return layout(near, head, far, placement, lead=lead, marks=list(zip(rel, val)), rng=rng)


# ---------------------------------------------------------------- the parse pass
def parse_batch(placement, mix, seed=0):
    """TCP segments of every kind of tests/_parse.py. wrap_frame: f is 24 bytes whose data offset says 40 — read with
    its low-word length the offset runs past the end; read as the span it is a header with four NOPs and then EOL.
    wrap_empty / straddle: the head is a plain header, which a zero-length reading calls too short."""
    rng = np.random.default_rng([0xFA2, PLACEMENTS.index(placement), MIXES.index(mix), seed])
    mp = _max_payload(mix, 60)
    near = [_parse.segment(rng, k, mp) for k in rng.choice(_parse.KINDS, N_NEAR)]
    far = [_parse.segment(rng, k, mp) for k in rng.choice(_parse.KINDS, N_FAR)]
    if placement[0] == "wrap_frame":
        f = bytearray(_parse._seg(rng, [O.Option(kind=1)] * 4, 0).bytes())
        assert len(f) == 24
        f[12] = 10
        head, placement = bytes(f), ("wrap_frame", 24)
    else:
        head = _parse._seg(rng, [], 200).bytes()
    return layout(near, head, far, placement, lead=int(rng.integers(4)), rng=rng)


def parse_model(r, low=False):
    if low:
        return _parse.expected(r.low_buf, r.low_offs)
    e = _parse.expected(r.buf, r.offs)
    e["data_off"] = shift_behind_span(r, e["data_off"])
    return e


# ---------------------------------------------------------------- receive coalescing
BRIDGE_NEAR, BRIDGE_FAR, BRIDGE_PAY = 5, 14, 48


def gro_batch(ipver, placement, mix, flow=False, seed=0):
    """(layout, valid): connections of in-order frames (tests/_gro.flow_case), back to back for the adjacency call and
    round-robin for the flow-keyed one, and one bridge connection whose frames end the near run, are the head f of a
    wrap_frame span, and start the far run (so in a straddle placement the frame across byte 2^32 is inside a merged
    run). Every valid bit is set, the span's too: the passes must find by themselves that the span is no member."""
    rng = np.random.default_rng([0xFA3, ipver, PLACEMENTS.index(placement), MIXES.index(mix), int(flow), seed])
    mp = _max_payload(mix, 60 if ipver == 6 else 40)

    def conns(total):
        out = []
        while total > 0:
            k = min(total, int(rng.integers(3, 12)))
            p = int(rng.integers(1, mp + 1))
            pays = [p] * (k - 1) + [int(rng.integers(1, p + 1))]  # a short tail ends the run
            out.append(_gro.case_frames(_gro.flow_case(rng, ipver, pays)))
            total -= k
        return _gro_flow.round_robin(out)[0] if flow else [f for c in out for f in c]

    bridge = _gro.case_frames(_gro.flow_case(rng, ipver, [BRIDGE_PAY] * (BRIDGE_NEAR + 1 + BRIDGE_FAR)))
    near = conns(N_NEAR - BRIDGE_NEAR) + bridge[:BRIDGE_NEAR]
    far = bridge[BRIDGE_NEAR + 1:] + conns(N_FAR - BRIDGE_FAR)
    f = bridge[BRIDGE_NEAR]
    if placement[0] == "wrap_frame":
        head, placement = f, ("wrap_frame", len(f))
    else:
        head = _junk_head(rng, 0x60 if ipver == 6 else 0x45)
    r = layout(near, head, far, placement, lead=int(rng.integers(4)), rng=rng)
    return r, np.ones(r.n, bool)


def gro_model(ipver, buf, offs, valid, flow=False):
    return (_gro_flow.gro_flow if flow else _gro.gro)(buf, offs, valid, ipver)


# ---------------------------------------------------------------- the NAT rewrite
def nat_batch(ipver, placement, mix, seed=0):
    """(layout, valid, table, slots, ttl_dec): frames of the transmit pass's model with random tuples and TTLs, a rule
    for about half of them. In every placement the span's head is a frame whose tuple has a rule and whose valid bit
    is set (the f of wrap_frame): it must stay as it is. One frame in 16 has its valid bit clear."""
    rng = np.random.default_rng([0xFA4, ipver, PLACEMENTS.index(placement), MIXES.index(mix), seed])
    mp = _max_payload(mix, 60 if ipver == 6 else 40)
    fr = _nat.frames(rng, ipver, rng.integers(0, mp + 1, N_NEAR + N_FAR))
    f = _nat.frames(rng, ipver, [100], ttl=200)[0]
    ruled = [x for x in fr if rng.integers(2)] + [f]
    match = [_nat.tuple_of(x, ipver) for x in ruled]
    assert len(set(match)) == len(match)
    new = _nat.random_tuples(rng, len(match), ipver)
    slots = 16
    while slots < 2 * len(match):
        slots *= 2
    table = _nat.build_table(ipver, match, new, slots)
    if placement[0] == "wrap_frame":
        placement = ("wrap_frame", len(f))
    r = layout(fr[:N_NEAR], f, fr[N_NEAR:], placement, lead=int(rng.integers(4)), rng=rng)
    valid = rng.integers(16, size=r.n) != 0
    valid[r.span] = True
    return r, valid, table, slots, 1


def nat_model(ipver, buf, offs, valid, table, slots, ttl_dec):
    return _nat.rewrite(buf, offs, valid, table, slots, ttl_dec, ipver)


# ---------------------------------------------------------------- the build passes: far output slots
BUILD_NEAR, BUILD_FAR = 200, 400
BUILD_D = TWO32 - (1 << 19)  # the twin's far slots start at 2^19 - 700; the near slots end below that


def build_slots(slot_len, n_near=BUILD_NEAR):
    """Output offsets for frames of slot_len[i] bytes each (multiples of 4): (device offsets, twin offsets), n + 1
    entries. The first n_near frames are packed from 0, the others from 2^32 - 700 upward, so one frame lies across
    byte 2^32; the gap between the two runs is allowed ("bytes between a padded frame and the next offset left as they
    were"). The twin's far slots are BUILD_D lower."""
    slot_len = np.asarray(slot_len, np.uint64)
    assert 0 < n_near < slot_len.size and not (slot_len & np.uint64(3)).any()
    start = np.zeros(slot_len.size + 1, np.uint64)
    start[1:n_near + 1] = np.cumsum(slot_len[:n_near])
    far0 = TWO32 - STRADDLE_BACK
    assert far0 % 4 == 0 and int(start[n_near]) <= far0 - BUILD_D
    start[n_near:] = np.uint64(far0) + np.concatenate([[0], np.cumsum(slot_len[n_near:])]).astype(np.uint64)
    twin = start.copy()
    twin[n_near:] -= np.uint64(BUILD_D)
    assert int(start[-1]) <= ARENA and len(crossing(start)) == 1
    return start, twin
