// dec_n1024_dfft.inc — the one copy of phases 3 + 4 of the n = 1024, k = 256
// reconstruct: the closed-form derivative at y < 256 and the FFT restricted to
// y < 256 on the four live registers.  A fragment, included inside the kernel
// function by dec_n1024.hip (the 8-wave kernel and its packed form) and by
// dec_n1024x_tile.inc (the 12 / 16-wave and ragged kernels); a textual
// fragment and not a function for dec_n1024x_tile.inc's reason: as an
// always-inlined function the same statements compile to other schedules.
//
// In scope at the point of inclusion:
//   s          the wave's group (S16) in layout C (r bit 0 = p8, bit 1 = p9,
//              bit 2 = p6, bit 3 = p7; lane = p0..p5) after IFFT stages 8-9
//   lane       the lane index
//   hi67, lo, hi47, lo01, hi27
//              the lane bits above each swap stage, and L(i), the table
//              address of step i = 2..11 built from them (each kernel's own:
//              the two table images are addressed differently)
//   DFFT_TAB(i, T)
//              a macro that fetches the subfield table of step i into T
// Out: ql[q], qh[q] (declared here), q = 0..3: the FFT's outputs
// y = 4 * lane + q.
//
// Phases 3 + 4a: formal derivative (poly_encoder.hpp:195-215) and FFT
// stages 9, 8 (afft, additive_fft.hpp:121-141) for the outputs y < 256 only.
// Those FFT stages keep the block at j = d, whose skew skews[d - 1] is
// 0xFFFF: a ^= b * skew is a no-op, so they pass c'[y] through for y < 256,
// and the derivative is needed at y < 256 only.  Its closed form
// c'[y] = c[y] ^ XOR_{b: y_b = 0} c[y | 2^b] there reads
//   c'[y] = c0[y] ^ c1[y] ^ c2[y] ^ XOR_{b < 8, y_b = 0} c0[y | 2^b]
// with c0 / c1 / c2 = registers 4 q / 4 q + 1 / 4 q + 2 (p8 p9 = 00 / 10 /
// 01), q bit 0 = p6, bit 1 = p7, lane bits = p0..p5.
// Lane-bit terms (lanes with p_b = 0 add the value of lane + 2^b): p2, p3
// by one row_shl DPP xor each whose bank mask leaves the p_b = 1 lanes
// untouched; p0, p1 by quad_perm DPP xors that hand the p_b = 1 lanes
// their own c0 instead of 0 (corrected once: c0 is kept where p0 ^ p1 = 0
// rather than xor'ed twice); p4, p5 by permlane swaps, masked.
    uint32_t ql[4], qh[4];
    {
      const uint32_t keep0 = ((lane ^ (lane >> 1)) & 1) ? 0u : 0xffffffffu;
      const uint32_t m4 = ((lane >> 4) & 1) ? 0u : 0xffffffffu;
      const uint32_t m5 = ((lane >> 5) & 1) ? 0u : 0xffffffffu;
      const auto lane_terms = [&](uint32_t c0, uint32_t acc) {
        acc ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(c0), 0xF5, 0xf, 0xf, false));  // quad [1,1,3,3]
        acc ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(c0), 0xEE, 0xf, 0xf, false));  // quad [2,3,2,3]
        acc ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(c0), 0x104, 0xf, 0x5, false));  // row_shl:4, banks 0, 2
        acc ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(c0), 0x108, 0xf, 0x3, false));  // row_shl:8, banks 0, 1
        acc = __builtin_amdgcn_bitop3_b32(acc, from_upper(c0, 4), m4, 0x78);  // acc ^ (x & m)
        acc = __builtin_amdgcn_bitop3_b32(acc, from_upper(c0, 5), m5, 0x78);
        return __builtin_amdgcn_bitop3_b32(acc, c0, keep0, 0x78);
      };
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t al = s.l[4 * q + 1] ^ s.l[4 * q + 2], ah = s.h[4 * q + 1] ^ s.h[4 * q + 2];
        if (!(q & 1)) {  // p6 = 0
          al ^= s.l[4 * (q | 1)];
          ah ^= s.h[4 * (q | 1)];
        }
        if (!(q & 2)) {  // p7 = 0
          al ^= s.l[4 * (q | 2)];
          ah ^= s.h[4 * (q | 2)];
        }
        ql[q] = lane_terms(s.l[4 * q], al);
        qh[q] = lane_terms(s.h[4 * q], ah);
      }
    }
    {
      // q bit0 = p6, bit1 = p7; lane bits = p0..p5.  Positions < 256 only.
      auto fb = [&](int a, int bb, const SubTab &T) {  // every stage >= SUB for y < 256
        mul_acc_sub(ql[bb], qh[bb], T, ql[a], qh[a]);
        ql[bb] ^= ql[a];
        qh[bb] ^= qh[a];
      };
      // stage 7 (block j = 128) and stage 6's first block (j = 64) have the
      // skew 0xFFFF at index 0 (additive_fft.hpp:129): b ^= a only
      const auto fx = [&](int a, int bb) {
        ql[bb] ^= ql[a];
        qh[bb] ^= qh[a];
      };
      SubTab T[2];
      DFFT_TAB(2, T[0]);
      DFFT_TAB(3, T[1]);
      fx(0, 2);  // stage 7
      fx(1, 3);
      fx(0, 1);  // stage 6
      fb(2, 3, T[0]);
      DFFT_TAB(4, T[0]);
      // q (p6, p7) <-> lane bits 4, 5 (p4, p5)
      swap_bit(ql[0], ql[1], 4, false);
      swap_bit(qh[0], qh[1], 4, false);
      swap_bit(ql[2], ql[3], 4, false);
      swap_bit(qh[2], qh[3], 4, false);
      swap_bit(ql[0], ql[2], 5, false);
      swap_bit(qh[0], qh[2], 5, false);
      swap_bit(ql[1], ql[3], 5, false);
      swap_bit(qh[1], qh[3], 5, false);
      // now q = (p4, p5); lane bits 0-3 = p0..p3, 4 = p6, 5 = p7
      fb(0, 2, T[1]);  // stage 5
      fb(1, 3, T[1]);
      DFFT_TAB(5, T[1]);
      fb(0, 1, T[0]);  // stage 4
      DFFT_TAB(6, T[0]);
      fb(2, 3, T[1]);
      DFFT_TAB(7, T[1]);
      // q (p4, p5) <-> lane bits 2, 3 (p2, p3)
      const bool l2 = (lane >> 2) & 1, l3 = (lane >> 3) & 1;
      swap_bit(ql[0], ql[1], 2, l2);
      swap_bit(qh[0], qh[1], 2, l2);
      swap_bit(ql[2], ql[3], 2, l2);
      swap_bit(qh[2], qh[3], 2, l2);
      swap_bit(ql[0], ql[2], 3, l3);
      swap_bit(qh[0], qh[2], 3, l3);
      swap_bit(ql[1], ql[3], 3, l3);
      swap_bit(qh[1], qh[3], 3, l3);
      // now q = (p2, p3); lane bits 0,1 = p0,p1; 2,3 = p4,p5; 4,5 = p6,p7
      fb(0, 2, T[0]);  // stage 3
      fb(1, 3, T[0]);
      DFFT_TAB(8, T[0]);
      fb(0, 1, T[1]);  // stage 2
      DFFT_TAB(9, T[1]);
      fb(2, 3, T[0]);
      DFFT_TAB(10, T[0]);
      // q (p2, p3) <-> lane bits 0, 1 (p0, p1)
      const bool l0 = lane & 1, l1 = (lane >> 1) & 1;
      swap_bit(ql[0], ql[1], 0, l0);
      swap_bit(qh[0], qh[1], 0, l0);
      swap_bit(ql[2], ql[3], 0, l0);
      swap_bit(qh[2], qh[3], 0, l0);
      swap_bit(ql[0], ql[2], 1, l1);
      swap_bit(qh[0], qh[2], 1, l1);
      swap_bit(ql[1], ql[3], 1, l1);
      swap_bit(qh[1], qh[3], 1, l1);
      // now q = (p0, p1); lane = (p2 .. p7): y = 4 * lane + q
      fb(0, 2, T[1]);  // stage 1
      fb(1, 3, T[1]);
      DFFT_TAB(11, T[1]);
      fb(0, 1, T[0]);  // stage 0
      fb(2, 3, T[1]);
    }
