"""Seeded random receive batches for UDP receive coalescing (tests/test_gpu_ugro_fuzz.py): a few hundred datagrams of
several flows, each flow a sequence of bursts cut as UDP segmentation offload cuts a super-datagram (k - 1 datagrams of
gso bytes and a tail), the flows interleaved in chunks, and a sprinkling of corrupt, padded and zero-checksum frames and
of clear valid bits. Every batch holds, by construction, a run of three or more datagrams that arrive back to back (the
first burst of the first flow opens the batch and is left alone) and at least one non-member (a padded datagram is
forced in where the sprinkling made none); tests/test_ugro_gen.py asserts both from the model for every seed in SEEDS.
No torch and no GPU at import."""
import numpy as np

import _udp
import _ugro

SEEDS = tuple(range(6))
GSOS = (1, 7, 33, 200, 536, 1472)
KINDS = ("payload_byte", "ip_header_bit", "field_zero", "udp_len_short", "udp_len_long", "udp_len_trim", "protocol",
         "length_field", "truncate", "version", "padding")


def _bursts(rng, frames, first_long):
    """Payload lengths of one flow, about `frames` of them, burst by burst; first_long: the first burst has at least
    three full datagrams before its tail. Returns (lengths, the first burst's size)."""
    pays, first = [], 0
    while len(pays) < frames:
        g = int(rng.choice(GSOS))
        k = int(rng.integers(4, 9)) if first_long and not pays else int(rng.integers(1, 9))
        tail = int(rng.integers(0, g + 1)) if rng.integers(4) else g
        pays += [g] * (k - 1) + [tail if k > 1 or tail else g]
        first = first or k
    return pays, first


def draw(seed: int, ipver: int):
    """(buf, offsets, valid, protected): valid = the bits the receive verify's model gives, less a few cleared ones;
    protected = the size of the first flow's first burst, which opens the batch and which nothing was done to."""
    rng = np.random.default_rng([0x06F2, ipver, seed])
    nflows = int(rng.integers(4, 10))
    total = int(rng.integers(150, 320))
    flows, protected = [], 0
    for k in range(nflows):
        pays, first = _bursts(rng, total // nflows + 1, first_long=k == 0)
        flows.append(_ugro.flow_frames(rng, ipver, pays))
        protected = protected or first
    frames = flows[0][:protected]
    at = [0] * nflows
    at[0] = protected
    while True:
        live = [k for k in range(nflows) if at[k] < len(flows[k])]
        if not live:
            break
        k = int(rng.choice(live))
        c = int(rng.integers(1, 7))
        frames += flows[k][at[k]:at[k] + c]
        at[k] += c
    n = len(frames)
    hit = False
    for i in range(protected, n):
        if rng.integers(12) == 0:
            frames[i] = bytes(_udp.corrupt(rng, np.frombuffer(frames[i], np.uint8), ipver, str(rng.choice(KINDS))))
            hit = True
    if not hit:
        i = int(rng.integers(protected, n))
        frames[i] = bytes(_udp.corrupt(rng, np.frombuffer(frames[i], np.uint8), ipver, "padding"))
    buf, offs = _ugro.pack(frames, lead=int(rng.integers(4)))
    valid, _, _ = _udp.rx_expected(ipver, buf, offs)
    clear = rng.integers(32, size=n) == 0
    clear[:protected] = False
    return buf, offs, valid & ~clear, protected
