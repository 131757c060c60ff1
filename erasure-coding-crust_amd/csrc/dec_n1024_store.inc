// dec_n1024_store.inc — the one copy of phase 5's column store of the
// n = 1024, k = 256 reconstruct: a fragment, included inside the kernel
// function by dec_n1024.hip and dec_n1024x_tile.inc (see dec_n1024_dfft.inc).
//
// In scope at the point of inclusion:
//   ol[q], oh[q]   the low / high bytes of the output rows y = 4 * lane + q,
//                  q = 0..3, of the group's 4 columns (byte c: column c)
//   cbase, ncols   the group's first column (wave-uniform), the item's columns
//   O, lane        the item's output, the lane index
// Column c of the group: 4 consecutive y -> 8 bytes BE of its 512-byte row.
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint64_t col = cbase + c;
        if (col >= ncols) break;
        const uint32_t w0 = vperm(ol[0], oh[0], 0x0c0c0400u + 0x0101u * c) |
                            (vperm(ol[1], oh[1], 0x0c0c0400u + 0x0101u * c) << 16);
        const uint32_t w1 = vperm(ol[2], oh[2], 0x0c0c0400u + 0x0101u * c) |
                            (vperm(ol[3], oh[3], 0x0c0c0400u + 0x0101u * c) << 16);
        *reinterpret_cast<uint2 *>(O + (col * K + 4 * lane) * 2) = make_uint2(w0, w1);
      }
