//go:build nsx

// Segmentation offload over the MI355X library (nsx_tso_ipv4_tcp_build_host /
// nsx_tso_ipv6_tcp_build_host). A sender holds, per connection, one header
// template, one option block and a run of payload far longer than one MSS; it
// hands those over as they are — one SuperSegment per connection — and the
// GPU cuts them into frames: the payload at the MSS, the sequence number
// advanced by it, FIN and PSH kept for the last frame and CWR for the first
// (Linux's tcp_gso_segment rule; SYN is merely copied, a sender does not
// offload SYN segments), the IPv4 identification counted up. Whole IPv4 / IPv6
// datagrams come back, header and TCP checksums in place. As in build_nsx.go,
// everything the C call reads or writes lies in one pinned block, which a
// SuperSender keeps across batches.
package tcp

/*
#include "nsx_csum.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"unsafe"
)

// SuperSegment is one connection's send: seg carries the header template, the
// options and the whole payload run (seg.data); the IP fields are copied to
// every frame (Ident counts up per frame).
type SuperSegment struct {
	seg      segment
	MSS      uint32 // payload bytes per frame (Linux gso_size), at least 1
	Src, Dst []byte // ip.Addr.Raw(): 4 bytes each for IPv4, 16 for IPv6
	Ident    uint16 // IPv4 identification of the first frame
	TTL      uint8  // TTL / hop limit
	TClass   uint8  // IPv6 traffic class
	Flow     uint32 // IPv6 flow label (low 20 bits)
}

// BuiltFrames holds a batch's datagrams in pinned host memory.
type BuiltFrames struct {
	out    []byte
	outOff []uint64
	flen   []int
	// First[s] is super-segment s's first frame; First[len] the frame count.
	First []uint64
	// Raw is each frame's TCP raw sum (pseudo-header ‖ image, field zero); 0
	// marks a frame that did not fit its IP length field and was not built.
	Raw []uint16
}

// Len returns the number of frames.
func (b *BuiltFrames) Len() int { return len(b.flen) }

// Frame returns frame f: a view into pinned memory, valid until the
// SuperSender's next Build or Close.
func (b *BuiltFrames) Frame(f int) []byte {
	o := b.outOff[f]
	return b.out[o : o+uint64(b.flen[f])]
}

// SuperSender cuts and builds batches of super-segments through one pinned
// block it keeps across calls.
type SuperSender struct {
	arena pinnedArena
	b     BuiltFrames
}

// NewSuperSender returns a SuperSender with an empty block.
func NewSuperSender() *SuperSender { return &SuperSender{} }

// Close releases the pinned block (and every batch built in it).
func (s *SuperSender) Close() { s.arena.free() }

// Build cuts sups into frames of IP version ipver (4 or 6) and builds them.
// numGPUs 0 = auto.
func (s *SuperSender) Build(ipver int, sups []SuperSegment, numGPUs int) (*BuiltFrames, error) {
	if err := buildSuper(&s.arena, &s.b, ipver, sups, numGPUs); err != nil {
		return nil, err
	}
	return &s.b, nil
}

func buildSuper(arena *pinnedArena, b *BuiltFrames, ipver int, sups []SuperSegment, numGPUs int) error {
	if ipver != 4 && ipver != 6 {
		return errors.New("ipver must be 4 or 6")
	}
	n := len(sups)
	alen, iph := uint64(4), uint64(20)
	if ipver == 6 {
		alen, iph = 16, 40
	}
	b.First = grow(b.First, n+1)
	b.First[0] = 0
	var nOpt, nData, nOut uint64
	optLen := make([]uint64, n)
	for i, s := range sups {
		if s.MSS == 0 || uint64(len(s.Src)) != alen || uint64(len(s.Dst)) != alen {
			return errors.New("super-segment with MSS 0 or an address of the wrong length")
		}
		for _, op := range s.seg.options {
			optLen[i] += uint64(len(op.bytes()))
		}
		d, m := uint64(len(s.seg.data)), uint64(s.MSS)
		cnt := (d + m - 1) / m
		if cnt == 0 {
			cnt = 1
		}
		b.First[i+1] = b.First[i] + cnt
		nOpt += optLen[i]
		nData += d
	}
	nf := int(b.First[n])
	b.outOff, b.flen, b.Raw = grow(b.outOff, nf+1), grow(b.flen, nf), grow(b.Raw, nf)
	b.outOff[0] = 0
	if nf == 0 {
		b.out = nil
		return nil
	}
	f := 0
	for i, s := range sups {
		d, m := uint64(len(s.seg.data)), uint64(s.MSS)
		for at := uint64(0); f < int(b.First[i+1]); f, at = f+1, at+m {
			dl := m
			if at+dl > d {
				dl = d - at
			}
			b.flen[f] = int(iph + uint64(C.nsx_tcp_wire_len(C.uint64_t(optLen[i]), C.uint64_t(dl))))
			b.outOff[f+1] = b.outOff[f] + alignUp(uint64(b.flen[f]), 4)
		}
	}
	nOut = b.outOff[nf]
	un, uf := uint64(n), uint64(nf)
	// one pinned block: the 8 TCP field arrays, the 6 IP field arrays, mss, data/opt offsets, frame_first,
	// frame_seg, out offsets, option bytes, payload bytes, frames, raw sums
	sizes := []uint64{2 * un, 2 * un, 4 * un, 4 * un, un, un, 2 * un, 2 * un,
		alen * un, alen * un, 2 * un, un, un, 4 * un, 4 * un,
		8 * (un + 1), 8 * (un + 1), 8 * (un + 1), 4 * uf, 8 * (uf + 1), nOpt + 1, nData + 1, nOut, 2 * uf}
	var at [25]uint64
	for k, sz := range sizes {
		at[k+1] = alignUp(at[k]+sz, 64)
	}
	if err := arena.reserve(at[len(sizes)], 0); err != nil {
		return err
	}
	region := func(k int) unsafe.Pointer { return unsafe.Pointer(&arena.buf[at[k]]) }
	srcPort := unsafe.Slice((*uint16)(region(0)), n)
	dstPort := unsafe.Slice((*uint16)(region(1)), n)
	seqNum := unsafe.Slice((*uint32)(region(2)), n)
	ackNum := unsafe.Slice((*uint32)(region(3)), n)
	offset := unsafe.Slice((*uint8)(region(4)), n)
	control := unsafe.Slice((*uint8)(region(5)), n)
	window := unsafe.Slice((*uint16)(region(6)), n)
	urgentPtr := unsafe.Slice((*uint16)(region(7)), n)
	src := unsafe.Slice((*byte)(region(8)), alen*un)
	dst := unsafe.Slice((*byte)(region(9)), alen*un)
	ident := unsafe.Slice((*uint16)(region(10)), n)
	ttl := unsafe.Slice((*uint8)(region(11)), n)
	tclass := unsafe.Slice((*uint8)(region(12)), n)
	flow := unsafe.Slice((*uint32)(region(13)), n)
	mss := unsafe.Slice((*uint32)(region(14)), n)
	dataOff := unsafe.Slice((*uint64)(region(15)), n+1)
	optOff := unsafe.Slice((*uint64)(region(16)), n+1)
	first := unsafe.Slice((*uint64)(region(17)), n+1)
	frameSeg := unsafe.Slice((*uint32)(region(18)), nf)
	outOff := unsafe.Slice((*uint64)(region(19)), nf+1)
	opts := unsafe.Slice((*byte)(region(20)), nOpt+1)
	data := unsafe.Slice((*byte)(region(21)), nData+1)
	b.out = unsafe.Slice((*byte)(region(22)), nOut)
	raw := unsafe.Slice((*uint16)(region(23)), nf)
	var d, o uint64
	for i, s := range sups {
		t := s.seg
		srcPort[i], dstPort[i], seqNum[i], ackNum[i] = t.srcPort, t.dstPort, t.seqNum, t.ackNum
		offset[i], control[i], window[i], urgentPtr[i] = t.offset, t.control.byte(), t.window, t.urgentPtr
		copy(src[alen*uint64(i):], s.Src)
		copy(dst[alen*uint64(i):], s.Dst)
		ident[i], ttl[i], tclass[i], flow[i], mss[i] = s.Ident, s.TTL, s.TClass, s.Flow, s.MSS
		dataOff[i], optOff[i], first[i] = d, o, b.First[i]
		for _, op := range t.options {
			o += uint64(copy(opts[o:], op.bytes()))
		}
		d += uint64(copy(data[d:], t.data))
		for k := b.First[i]; k < b.First[i+1]; k++ {
			frameSeg[k] = uint32(i)
		}
	}
	dataOff[n], optOff[n], first[n] = d, o, b.First[n]
	copy(outOff, b.outOff)

	var h C.nsx_tcp_hdr_soa
	h.src_port = (*C.uint16_t)(region(0))
	h.dst_port = (*C.uint16_t)(region(1))
	h.seq_num = (*C.uint32_t)(region(2))
	h.ack_num = (*C.uint32_t)(region(3))
	h.offset = (*C.uint8_t)(region(4))
	h.control = (*C.uint8_t)(region(5))
	h.window = (*C.uint16_t)(region(6))
	h.urgent_ptr = (*C.uint16_t)(region(7))
	var ip C.nsx_ip_hdr_soa
	ip.src = (*C.uint8_t)(region(8))
	ip.dst = (*C.uint8_t)(region(9))
	ip.ident = (*C.uint16_t)(region(10))
	ip.ttl = (*C.uint8_t)(region(11))
	ip.tclass = (*C.uint8_t)(region(12))
	ip.flow = (*C.uint32_t)(region(13))
	var optOffs *C.uint64_t
	if nOpt > 0 {
		optOffs = (*C.uint64_t)(region(16))
	}
	var rc C.int
	if ipver == 4 {
		rc = C.nsx_tso_ipv4_tcp_build_host(&ip, &h, (*C.uint8_t)(region(20)), optOffs, (*C.uint8_t)(region(21)),
			(*C.uint64_t)(region(15)), (*C.uint32_t)(region(14)), C.uint64_t(n), (*C.uint64_t)(region(17)),
			(*C.uint32_t)(region(18)), C.uint64_t(nf), (*C.uint8_t)(region(22)), (*C.uint64_t)(region(19)),
			(*C.uint16_t)(region(23)), C.int(numGPUs))
	} else {
		rc = C.nsx_tso_ipv6_tcp_build_host(&ip, &h, (*C.uint8_t)(region(20)), optOffs, (*C.uint8_t)(region(21)),
			(*C.uint64_t)(region(15)), (*C.uint32_t)(region(14)), C.uint64_t(n), (*C.uint64_t)(region(17)),
			(*C.uint32_t)(region(18)), C.uint64_t(nf), (*C.uint8_t)(region(22)), (*C.uint64_t)(region(19)),
			(*C.uint16_t)(region(23)), C.int(numGPUs))
	}
	if rc != C.NSX_OK {
		b.out = nil
		return fmt.Errorf("nsx_tso_ipv%d_tcp_build_host: %s", ipver, C.GoString(C.nsx_strerror(rc)))
	}
	copy(b.Raw, raw)
	return nil
}
