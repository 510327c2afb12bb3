// dec_unfilter_body.inc -- the body of dec_unfilter_kernel<kLayout> and of dec_unfilter_planar_kernel (decode.hip includes it once in
// each).  It is text, not a __device__ template: called through a function, the packed and layout kernels no longer compile to the
// instructions they had (registers and schedule move: tools/isa_diff.py), and they are frozen.  The including kernel provides
//   kLayout, kPlanar   constexpr bool: DecJob::sel / pitch destinations; planes (dst_c planes of w-byte rows, DecJob::pitch between a
//                      plane's rows, plane_pitch[file] between the planes).  Only the last stage ("the pixels") differs.
//   plane_pitch        const int64_t *, a word per file of `jobs` (kPlanar; else a null constant that is never read)
//   kVerify            constexpr bool: the tile also sums its filtered bytes for the file's Adler-32 (fpng_amd_encoder_set_decode_verify);
//                      false in the three kernels that were there before, whose instructions it leaves alone
//   adler_acc          unsigned long long *, two words per file of `jobs` (kVerify; else a null constant that is never read)
//   kFloat             constexpr int: -1, or (kPlanar) the FPNG_AMD_F32 / F16 / BF16 of fpng_amd_decode_batch_planar_float -- the planes
//                      hold elements of that type, fmaf(value, flt.scale[c], flt.bias[c]) of the file's channel c; -1 in the kernels
//                      that were there before, whose instructions it leaves alone
//   flt                DecFloat, a kernel argument: wave-uniform (kFloat >= 0; else an empty constant that is never read)
//   kCrop              constexpr bool (kPlanar): the planes hold a crop of the file (fpng_amd_decode_batch_planar_crop) -- the plan numbers only
//                      the tiles the crop needs (dec_crop_tiles; all of them where kVerify), tiles and waves that hold none of its
//                      pixels leave once their look-back granules are published, and the last stage clips to the crop; false in the
//                      kernels that were there before, whose instructions it leaves alone
//   crops              const DecCrop *, a record per file of `jobs` (kCrop; else a null constant that is never read)
// and the kernel's arguments jobs, plan, placed, item0, status, epoch, skip_mask.
    __shared__ __attribute__((aligned(16))) uint8_t tile_mem[kUnfRows * kTilePitch];
    __shared__ uint32_t mask_mem[kUnfRows * kRowMaskWords], epx_mem[kUnfRows]; // the rows' marked pixels (long matches), their entry pixels
    __shared__ uint32_t s_first[kWave + 1], s_i0[kWave], s_res[3 * kWave];      // the tile's walks (fill_tile)
    FPNG_TILE_STAMP(0);
    // Items are numbered SEGMENT by segment across all files of the group: the files, sorted by their segment counts (most
    // first), form `pieces` of segments over which the set of files that still have rows is constant -- its first `alive` ones,
    // cbpre[] = their column blocks' prefix sums.  One workgroup per item, item = workgroup number: an item waits for items with
    // LOWER numbers only, and the hardware starts the workgroups of a grid in rising order (per XCD, each XCD taking a fixed share
    // of the numbers: the lowest unfinished item is then always running or next in line for a free slot).  Measured alternatives,
    // 8 x 8K: tickets drawn from one atomic counter 1.72 ms, from one counter per column block 0.78 ms, persistent workgroups
    // taking their items in rising order 0.89 ms, this 0.54 ms, the former two kernels (sums, then a second read) 0.88 ms.  A spin
    // that does not end -- it cannot, unless workgroups do not start in that order after all -- gives up after kSpinLimit polls
    // and leaves the file to the CPU decoder (FPNG_AMD_DECODE_UNDECIDED).
    constexpr uint32_t kSpinLimit = 1u << 20;
    {
        // Which item?  The hardware deals a grid's workgroups to the eight XCDs in turn, and neighbouring items -- the column blocks of
        // one band of rows -- read the same blocks of token records where their windows meet: inside every run of 64 workgroups the
        // numbers are dealt so that eight neighbours share an XCD, i.e. an L2.  (Items still wait for lower numbers only; the order of
        // the runs is the grid's.)
        const uint32_t b = blockIdx.x, b_run = b & ~63u;
        const uint32_t item = item0 + (b_run + 64u <= gridDim.x ? b_run + ((b & 7u) << 3) + ((b >> 3) & 7u) : b); // (item0: a later launch for the same files, fpng_amd_decode_host's streamed form)
        if (item >= plan.total_items) return;
        // (which piece, which file: the lists are short -- eight files, one piece -- and a binary search over them in memory is a chain of
        //  round trips in front of everything else the tile does: the lanes of a wave look at an element each, all at once)
        const uint32_t l64 = threadIdx.x & (kWave - 1);
        DecUnfPiece pc;
        uint32_t per_seg, fidx, cb0, ji_w = 0xFFFFFFFFu;
        if (plan.n_pieces <= (uint32_t)kWave && plan.n_files < (uint32_t)kWave) {
            const bool hasp = l64 < plan.n_pieces, hasf = l64 <= plan.n_files;
            const DecUnfPiece mine = plan.pieces[hasp ? l64 : 0u];
            const uint32_t cbl = plan.cbpre[hasf ? l64 : 0u], ordl = plan.order[l64 < plan.n_files ? l64 : 0u];
            const uint32_t pi = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(hasp && mine.item0 <= item)) - 1u; // (pieces rise; the first one begins at item 0)
            pc.item0 = (uint32_t)__builtin_amdgcn_readlane((int)mine.item0, (int)pi), pc.seg0 = (uint32_t)__builtin_amdgcn_readlane((int)mine.seg0, (int)pi);
            pc.alive = (uint32_t)__builtin_amdgcn_readlane((int)mine.alive, (int)pi), pc.pad_ = 0;
            per_seg = (uint32_t)__builtin_amdgcn_readlane((int)cbl, (int)pc.alive);
            const uint32_t within0 = (item - pc.item0) % per_seg;
            fidx = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(l64 < pc.alive && cbl <= within0)) - 1u;
            cb0 = (uint32_t)__builtin_amdgcn_readlane((int)cbl, (int)fidx);
            ji_w = (uint32_t)__builtin_amdgcn_readlane((int)ordl, (int)fidx);
        } else {
            uint32_t lo = 0, hi = plan.n_pieces;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (plan.pieces[mid].item0 <= item) lo = mid; else hi = mid;
            }
            pc = plan.pieces[lo];
            per_seg = plan.cbpre[pc.alive];
            const uint32_t within0 = (item - pc.item0) % per_seg;
            lo = 0, hi = pc.alive;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (plan.cbpre[mid] <= within0) lo = mid; else hi = mid;
            }
            fidx = lo, cb0 = plan.cbpre[lo];
        }
        const uint32_t rel = item - pc.item0, sg = uni32(pc.seg0 + rel / per_seg), within = rel % per_seg;
        const uint32_t ji = ji_w != 0xFFFFFFFFu ? ji_w : uni32(plan.order[fidx]);
        // (kCrop: the crop's four words, wave-uniform like the job's; the plan counts column blocks from the crop's first one --
        //  from the file's where every tile runs for the Adler-32)
        static_assert(!kCrop || kPlanar, "crops are planar destinations");
        DecCrop crop = {};
        if constexpr (kCrop) {
            crop = crops[ji];
            crop.x = uni32(crop.x), crop.y = uni32(crop.y), crop.w = uni32(crop.w), crop.h = uni32(crop.h);
        }
        const uint32_t cb = uni32(within - cb0) + (kCrop && !kVerify ? dec_crop_first_block(crop.x) : 0u);
        // (the file's record, read by every lane, into scalar registers: the compiler keeps what it loads from writable global
        //  memory in vector registers, and every address derived from it would cost a register pair per row)
        DecJob job = jobs[ji];
        job.win = (uint32_t *)uni64((uint64_t)(uintptr_t)job.win), job.out = (uint8_t *)uni64((uint64_t)(uintptr_t)job.out);
        job.segsum = (uint32_t *)uni64((uint64_t)(uintptr_t)job.segsum);
        job.sub_base = uni32(job.sub_base);
        job.w = uni32(job.w), job.h = uni32(job.h), job.bpl = uni32(job.bpl), job.src_c = uni32(job.src_c), job.dst_c = uni32(job.dst_c), job.nseg = uni32(job.nseg), job.mode = uni32(job.mode);
        if constexpr (kLayout) job.sel = uni32(job.sel), job.pitch = (int32_t)uni32((uint32_t)job.pitch);
        if constexpr (kPlanar) job.pitch = (int32_t)uni32((uint32_t)job.pitch);
        // (only bits that the kernels in FRONT of this one set decide: every workgroup must come to the same conclusion about a
        //  file, or a later segment would wait for an earlier one that was skipped.  This kernel's own findings -- the tile's walk,
        //  the filter bytes, the look-back -- set other bits (decode.h: kDecTile*, kDecBadFilter; the static_assert there keeps them
        //  out of kDecUnfSkipMask), so the word's skip bits are the same for every thread of the launch.  skip_mask = kDecUnfSkipMask;
        //  0 where kernels that set those bits run NEXT to this launch -- the streamed form undoes a piece's rows on a stream of its
        //  own while the next piece is decoded: there every workgroup runs and publishes, whatever the status word says by then; a
        //  damaged file's rows are garbage either way and its status says so)
        if (job.mode != 0 || (status[ji] & skip_mask)) return;
        const uint32_t ncol = (job.bpl + 3) / 4;
        const uint32_t sc = job.src_c, dc = job.dst_c, lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
        // Which dword column is this thread's?  Rows of 4-byte pixels: workgroup-thread t has column cb * 256 + t.  Rows of 3-byte
        // pixels: a wave takes 48 dword columns = 192 bytes = 64 WHOLE pixels (its lanes 48..63 hold no column), a column block is
        // 256 pixels either way; where such rows become 4-channel pixels every lane writes one pixel, gathered from two lanes'
        // dwords -- dword stores instead of a byte at a time.
        const bool three = sc == 3, widen = three && dc == 4;
        const uint32_t wave_px = (cb * (kDecBlock / kWave) + wv) * kWave; // (the wave's first pixel)
        const uint32_t j4 = three ? (wave_px / 4) * 3 + lane : cb * kDecBlock + threadIdx.x;
        const bool active = j4 < ncol && (!three || lane < 48) && threadIdx.x < (uint32_t)kDecBlock;
        const uint32_t y0 = sg * kUnfRows, nrows = min(kUnfRows, job.h - y0);
        // ---- the tile's rows, from the token records (all threads; the barriers stand in front of every way out) ----
        lds_u8 *tile = (lds_u8 *)tile_mem;
        {
            const uint32_t ncb = dec_col_blocks(job.w, sc, dc), cbw = dec_col_block_bytes(sc, dc), last_sub = placed.eob_index[ji];
            lds_u32 *bm = (lds_u32 *)mask_mem, *epx = (lds_u32 *)epx_mem;
            const uint32_t err = sc == 4 ? fill_tile<4>(job, placed, last_sub, y0, nrows, cb, ncb, cbw, tile, bm, epx, s_first, s_i0, s_res, item0)
                                         : fill_tile<3>(job, placed, last_sub, y0, nrows, cb, ncb, cbw, tile, bm, epx, s_first, s_i0, s_res, item0);
            if (err) atomicOr(&status[ji], (err & kEmitBadStream ? kDecTileBadStream : 0u) | (err & kEmitLeaveToCpu ? kDecTileLeaveToCpu : 0u));
            __syncthreads();
            if (sc == 4) propagate_matches<4>(tile, bm, epx, nrows, s_i0); else propagate_matches<3>(tile, bm, epx, nrows, s_i0);
        }
        __syncthreads();
        FPNG_TILE_STAMP(1);
        if (threadIdx.x >= (uint32_t)kDecBlock) return; // (the tile is filled: from here on a thread per dword column)
        if (cb == 0 && threadIdx.x == 0) {
            bool bad = false;
            for (uint32_t k = 0; k < nrows; k++) bad |= tile[k * kTilePitch + kTileData - 1] != (y0 + k ? 2 : 0);
            if (bad) atomicOr(&status[ji], kDecBadFilter);
        }
        if (!kPlanar && !widen && !active) return; // (the lanes of a widening wave all stay: they write pixels; so do a planar wave's, each other's sources)
        if ((kPlanar || widen) && wave_px >= job.w) return;
        // ---- the columns' running sums, in place: row k of the tile becomes the sum of its rows 0 .. k (every thread its own dword
        //      column; eight rows in flight).  The rows stay in LDS -- until round 6 a thread held its 48 of them in registers, which
        //      is what kept the kernel at four waves per SIMD. ----
        lds_u32 *T = (lds_u32 *)(tile + kTileData) + (three ? wv * 48 + lane : threadIdx.x); // this thread's dword column of the tile
        constexpr uint32_t P = kTilePitch / 4;
        uint32_t p = 0;
        // (kVerify) The Adler-32 of the filtered stream, from the dwords this loop holds anyway: s1 = the bytes' sum, s2 = their sum
        // weighted with N - i, the bytes from byte i of the stream to its end (N = (bpl + 1) * h; the byte at row y, offset j of
        // the row's data is i = y * (bpl + 1) + 1 + j).  A dword's four weights are vw3 + 3, + 2, + 1, + 0 with vw3 the weight of
        // its last byte mod 65521 (bytes past the row's end are masked to zero: theirs does not matter): vw3 * (sum of the bytes)
        // + (3, 2, 1, 0) . bytes, at most 65520 * 1020 + 1530 a dword -- 48 rows of them fit 32 bits.  The filter bytes
        // (checked above: kDecBadFilter) are added in closed form by dec_verify_kernel.
        uint32_t vs1 = 0, vs2 = 0, vw3 = 0, vstep = 0, vmask = 0;
        if constexpr (kVerify) {
            static_assert(kUnfRows <= 64, "a thread's weighted sum must fit 32 bits");
            const uint64_t stride = (uint64_t)job.bpl + 1;
            const uint32_t row_m = (uint32_t)((stride * (job.h - y0) - 1) % kAdlerMod); // N - (y0 * stride + 1): the weight of row y0's first data byte
            vw3 = (row_m + kAdlerMod - (4u * j4 + 3u) % kAdlerMod) % kAdlerMod;
            vstep = (uint32_t)(stride % kAdlerMod);
            const uint32_t nbv = active ? min(4u, job.bpl - 4u * j4) : 0u;
            vmask = nbv == 4 ? 0xFFFFFFFFu : (1u << (8 * nbv)) - 1u;
        }
        if (active) {
            for (uint32_t k = 0; k < nrows; k += 8) {
                uint32_t t8[8];
#pragma unroll
                for (uint32_t q = 0; q < 8; q++) t8[q] = T[min(k + q, nrows - 1) * P];
#pragma unroll
                for (uint32_t q = 0; q < 8; q++)
                    if (k + q < nrows) {
                        if constexpr (kVerify) {
                            const uint32_t v = t8[q] & vmask, bs = __builtin_amdgcn_sad_u8(v, 0u, 0u);
                            vs1 += bs;
                            vs2 += vw3 * bs + 3u * (v & 0xFFu) + 2u * ((v >> 8) & 0xFFu) + ((v >> 16) & 0xFFu);
                            vw3 = vw3 >= vstep ? vw3 - vstep : vw3 + kAdlerMod - vstep;
                        }
                        p = add_bytes(p, t8[q]), T[(k + q) * P] = p;
                    }
            }
        }
        if constexpr (kVerify) {
            // The lanes that are still here form a prefix of the wave (lanes without a column have left, or -- where pixels are
            // widened or planes written -- all 64 have stayed): a reduction towards lane 0 through lanes that exist, then one
            // atomic add per sum and wave.  Integer adds commute: the file's sums do not depend on the order of the tiles.
            const uint32_t alive = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(true));
            vs2 %= kAdlerMod;
#pragma unroll
            for (uint32_t o = 32; o; o >>= 1) {
                const uint32_t a1 = (uint32_t)__shfl_down((int)vs1, o, kWave), a2 = (uint32_t)__shfl_down((int)vs2, o, kWave);
                if (lane + o < alive) vs1 += a1, vs2 += a2;
            }
            if (lane == 0 && (vs1 | vs2)) {
                atomicAdd(&adler_acc[2 * (size_t)ji], (unsigned long long)vs1);
                atomicAdd(&adler_acc[2 * (size_t)ji + 1], (unsigned long long)vs2);
            }
        }
        FPNG_TILE_STAMP(2);
        gu64 *gran = (gu64 *)(uintptr_t)job.segsum + j4;
        uint32_t carry = 0;
        if (active && (sg + 1 < job.nseg || sg)) { // (a file of one segment publishes nothing)
            gu64 *mine = gran + (size_t)sg * ncol;
            if (sg == 0)
                __hip_atomic_store(mine, ((unsigned long long)(epoch << 2 | 2u) << 32) | p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else {
                if (sg + 1 < job.nseg) __hip_atomic_store(mine, ((unsigned long long)(epoch << 2 | 1u) << 32) | p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                bool stalled = false;
                for (uint32_t q = sg; q-- > 0 && !stalled;) {
                    gu64 *g = gran + (size_t)q * ncol;
                    unsigned long long x = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    for (uint32_t spins = 0; (uint32_t)(x >> 34) != epoch; spins++) {
                        if (spins == kSpinLimit) {
                            stalled = true;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                        x = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    carry = add_bytes(carry, (uint32_t)x);
                    if (((uint32_t)(x >> 32) & 3u) == 2u) break;
                }
                if (stalled) atomicOr(&status[ji], kDecTileStalled);
                if (sg + 1 < job.nseg)
                    __hip_atomic_store(mine, ((unsigned long long)(epoch << 2 | 2u) << 32) | add_bytes(carry, p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if constexpr (kCrop) {
            // (published: nothing below waits for this tile any more.  A tile above or below the crop's rows has no pixels to write,
            //  nor has a wave whose 64 pixels lie beside its columns -- the whole wave leaves, its lanes are each other's sources)
            if (y0 + nrows <= crop.y || y0 >= crop.y + crop.h) return;
            if (wave_px >= crop.x + crop.w || wave_px + (uint32_t)kWave <= crop.x) return;
        }
        // ---- the pixels.  Dword stores at any byte address (rows of 3-channel pixels start anywhere; the hardware takes
        //      unaligned dwords, as it does for the loads above); bytes only where a row ends inside a dword ----
        FPNG_TILE_STAMP(3);
        const size_t os = (size_t)job.w * dc;
        gu8 *orow = (gu8 *)(uintptr_t)(job.out + (kLayout ? (int64_t)y0 * job.pitch : (int64_t)((size_t)y0 * os)));
        auto row = [&](uint32_t k) -> gu8 * { // (layout jobs: a signed pitch, negative for bottom-up rows)
            if constexpr (kLayout) return orow + (int64_t)k * job.pitch;
            else return orow + (size_t)k * os;
        };
        auto row_sum = [&](uint32_t k) { return active ? add_bytes(carry, T[k * P]) : 0u; }; // the pixels' bytes of row k, this thread's four
        // (layout jobs: a pixel dword in R,G,B,A order -> the destination's byte order, X bytes 0xFF)
        auto reorder = [&](uint32_t v) {
            if constexpr (kLayout) return __builtin_amdgcn_perm(0u, v, job.sel);
            else return v;
        };
        if constexpr (kPlanar) {
            // Planes: a byte transpose inside the wave, after which a lane holds FOUR consecutive pixels' bytes of ONE channel and
            // stores them as a dword into that channel's plane (at any byte address; bytes only where the row ends inside it).
            const int64_t pp = (int64_t)uni64((uint64_t)plane_pitch[ji]);
            uint32_t ch, x; // this lane's plane, and the first of its four pixels
            if (three) ch = lane >> 4, x = wave_px + 4u * (lane & 15u);
            else ch = lane & 3u, x = wave_px + (lane & ~3u);
            const uint32_t nb = (ch < dc && x < job.w) ? min(4u, job.w - x) : 0u;
            constexpr uint32_t kElem = kFloat < 0 ? 1u : dec_float_bytes((uint32_t)kFloat); // bytes of a plane's element (the pitches are bytes)
            // (kCrop: the destination's row 0 is the file's row crop.y, its column 0 the file's column crop.x -- both differences may
            //  be negative here, the clipping below keeps every store inside; keep: bit e = the lane's pixel x + e lies in the crop's
            //  columns, cut at BOTH ends; k_lo .. k_hi: the tile's rows that lie in the crop's)
            gu8 *pb = (gu8 *)(uintptr_t)(job.out + (int64_t)ch * pp + ((int64_t)y0 - (int64_t)crop.y) * job.pitch + ((int64_t)x - (int64_t)crop.x) * kElem);
            uint32_t keep = 0;
            if constexpr (kCrop) {
                const uint32_t c_lo = max(x, crop.x) - x, c_hi = min(x + 4u, crop.x + crop.w) - x; // (the wave meets the crop; a lane beside it: c_lo >= c_hi, mod 2^32)
                if (ch < dc && x < crop.x + crop.w && x + 4u > crop.x) keep = (0xFu << c_lo) & (0xFu >> (4u - c_hi));
            }
            const uint32_t k_lo = kCrop ? max(crop.y, y0) - y0 : 0u, k_hi = kCrop ? min(crop.y + crop.h, y0 + nrows) - y0 : nrows;
            // (kFloat: the lane's channel's two constants, picked once from the four pairs in scalar registers)
            const float fs = kFloat < 0 ? 0.f : (ch == 0 ? flt.scale[0] : (ch == 1 ? flt.scale[1] : (ch == 2 ? flt.scale[2] : flt.scale[3])));
            const float fb = kFloat < 0 ? 0.f : (ch == 0 ? flt.bias[0] : (ch == 1 ? flt.bias[1] : (ch == 2 ? flt.bias[2] : flt.bias[3])));
            auto put = [&](uint32_t k, uint32_t d) {
                gu8 *q = pb + (int64_t)k * job.pitch;
                if constexpr (kCrop) {
                    // a whole quad as one store, as below; a quad cut at the front or the back as single elements
                    if constexpr (kFloat >= 0) {
                        const float f0 = __builtin_fmaf((float)(d & 0xFFu), fs, fb), f1 = __builtin_fmaf((float)((d >> 8) & 0xFFu), fs, fb);
                        const float f2 = __builtin_fmaf((float)((d >> 16) & 0xFFu), fs, fb), f3 = __builtin_fmaf((float)(d >> 24), fs, fb);
                        if constexpr (kFloat == 0) {
                            if (keep == 0xFu) *(gf32x4_any *)q = f32x4{f0, f1, f2, f3};
                            else if (keep) {
                                if (keep & 1u) *(gf32_any *)q = f0;
                                if (keep & 2u) *(gf32_any *)(q + 4) = f1;
                                if (keep & 4u) *(gf32_any *)(q + 8) = f2;
                                if (keep & 8u) *(gf32_any *)(q + 12) = f3;
                            }
                        } else {
                            const uint32_t lo = pack_half2<kFloat>(f0, f1), hi = pack_half2<kFloat>(f2, f3);
                            if (keep == 0xFu) *(gu32x2_any *)q = u32x2{lo, hi};
                            else if (keep) {
                                if (keep & 1u) *(gu16_any *)q = (uint16_t)lo;
                                if (keep & 2u) *(gu16_any *)(q + 2) = (uint16_t)(lo >> 16);
                                if (keep & 4u) *(gu16_any *)(q + 4) = (uint16_t)hi;
                                if (keep & 8u) *(gu16_any *)(q + 6) = (uint16_t)(hi >> 16);
                            }
                        }
                    } else if (keep == 0xFu) *(gu32_any *)q = d;
                    else if (keep) {
                        if (keep & 1u) q[0] = (uint8_t)d;
                        if (keep & 2u) q[1] = (uint8_t)(d >> 8);
                        if (keep & 4u) q[2] = (uint8_t)(d >> 16);
                        if (keep & 8u) q[3] = (uint8_t)(d >> 24);
                    }
                } else if constexpr (kFloat >= 0) {
                    // the dword's four bytes -> floats (v_cvt_f32_ubyte0 .. 3), ONE fused multiply-add each, then 16 (f32) or 8 bytes
                    // per lane (f16, bf16: packed conversions, round to nearest even); elements only where the row ends inside them
                    const float f0 = __builtin_fmaf((float)(d & 0xFFu), fs, fb), f1 = __builtin_fmaf((float)((d >> 8) & 0xFFu), fs, fb);
                    const float f2 = __builtin_fmaf((float)((d >> 16) & 0xFFu), fs, fb), f3 = __builtin_fmaf((float)(d >> 24), fs, fb);
                    if constexpr (kFloat == 0) {
                        if (nb == 4) *(gf32x4_any *)q = f32x4{f0, f1, f2, f3};
                        else if (nb) {
                            *(gf32_any *)q = f0;
                            if (nb > 1) *(gf32_any *)(q + 4) = f1;
                            if (nb > 2) *(gf32_any *)(q + 8) = f2;
                        }
                    } else {
                        const uint32_t lo = pack_half2<kFloat>(f0, f1), hi = pack_half2<kFloat>(f2, f3);
                        if (nb == 4) *(gu32x2_any *)q = u32x2{lo, hi};
                        else if (nb) {
                            *(gu16_any *)q = (uint16_t)lo;
                            if (nb > 1) *(gu16_any *)(q + 2) = (uint16_t)(lo >> 16);
                            if (nb > 2) *(gu16_any *)(q + 4) = (uint16_t)hi;
                        }
                    }
                } else if (nb == 4) *(gu32_any *)q = d;
                else
                    for (uint32_t b = 0; b < nb; b++) q[b] = (uint8_t)(d >> (8 * b));
            };
            if (three) {
                // lane L < 48 builds dword L % 16 of plane L / 16: bytes 12 d + ch + {0, 3, 6, 9} of the wave's 192, in the dwords of
                // lanes 3 d, 3 d + 1, 3 d + 2; lanes 48 .. 63 (four planes): 0xFF for the A plane
                const uint32_t d3 = 3u * (lane & 15u);
                const int la = (int)(d3 << 2), lb = (int)((d3 + 1) << 2), lc = (int)((d3 + 2) << 2);
                const uint32_t s1 = ch == 0 ? 0x0c060300u : (ch == 1 ? 0x0c070401u : 0x0c0c0502u), s2 = ch == 0 ? 0x05020100u : (ch == 1 ? 0x06020100u : 0x07040100u);
                for (uint32_t k = k_lo; k < k_hi; k++) {
                    const uint32_t v = row_sum(k);
                    const uint32_t a = (uint32_t)__builtin_amdgcn_ds_bpermute(la, (int)v), b = (uint32_t)__builtin_amdgcn_ds_bpermute(lb, (int)v), c = (uint32_t)__builtin_amdgcn_ds_bpermute(lc, (int)v);
                    const uint32_t d = ch == 3 ? 0xFFFFFFFFu : __builtin_amdgcn_perm(c, __builtin_amdgcn_perm(b, a, s1), s2);
                    put(k, d);
                }
            } else {
                // a thread holds one pixel: 4 x 4 bytes transposed inside every quad of lanes (DPP broadcasts of the quad's four
                // dwords stay in the VALU), lane 4 q + ch then holds channel ch of pixels 4 q .. 4 q + 3
                const uint32_t sq = ch | (4u + ch) << 8 | 0x0c0c0000u;
                for (uint32_t k = k_lo; k < k_hi; k++) {
                    const uint32_t v = row_sum(k);
                    const uint32_t v0 = quad_bcast<0>(v), v1 = quad_bcast<1>(v), v2 = quad_bcast<2>(v), v3 = quad_bcast<3>(v);
                    put(k, __builtin_amdgcn_perm(__builtin_amdgcn_perm(v3, v2, sq), __builtin_amdgcn_perm(v1, v0, sq), 0x05040100u));
                }
            }
        } else if (kLayout && sc == 3 && dc == 3 && job.sel != kDecSelRGB) {
            // 3 -> 3 bytes, B and R swapped: lane L holds bytes 4L .. 4L + 3 of the wave's 192 (64 whole pixels), and output byte i
            // is input byte i + 2, i or i - 2 as i is the first, second or third byte of its pixel -- for L % 3 = m the offsets
            // are (2, 1, 0, 5), (0, -1, 4, 3), (-2, 3, 2, 1) from 4L: two neighbours' dwords (the wave's first and last lanes need
            // none past the wave's ends), an 8-byte window out of the three, one v_perm_b32.  All lanes of the row come along:
            // they are each other's sources, the last one's bytes only where the row ends inside its dword.
            const uint32_t nb = min(4u, job.bpl - j4 * 4), m = lane % 3u;
            const uint32_t sh = m == 1 ? 24u : 0u, selm = m == 0 ? 0x05000102u : (m == 1 ? 0x04050001u : 0x05060702u);
            const int prev_l = (int)(((lane - 1u) & 63u) << 2), next_l = (int)(((lane + 1u) & 63u) << 2);
            const bool ragged = __builtin_amdgcn_ballot_w64(nb != 4) != 0;
            for (uint32_t k = 0; k < nrows; k++) {
                const uint32_t v = row_sum(k);
                const uint32_t prev = (uint32_t)__builtin_amdgcn_ds_bpermute(prev_l, (int)v), next = (uint32_t)__builtin_amdgcn_ds_bpermute(next_l, (int)v);
                const uint32_t a = m ? prev : v, b = m ? v : next; // the window: bytes 0 .. 7 of b:a from byte sh / 8
                const uint32_t d = __builtin_amdgcn_perm(funnel(next, b, sh), funnel(b, a, sh), selm);
                if (nb == 4) gstore_u32(row(k), j4 * 4, d);
                if (ragged && nb != 4)
                    for (uint32_t q = 0; q < nb; q++) gstore_u8(row(k), j4 * 4 + q, d >> (8 * q));
            }
        } else if (sc == dc) {
            const uint32_t nb = min(4u, job.bpl - j4 * 4);
            if (nb == 4) {
                for (uint32_t k = 0; k < nrows; k++) gstore_u32(row(k), j4 * 4, kLayout && sc == 4 ? reorder(row_sum(k)) : row_sum(k));
            } else {
                for (uint32_t k = 0; k < nrows; k++) {
                    const uint32_t v = row_sum(k);
                    for (uint32_t b = 0; b < nb; b++) gstore_u8(row(k), j4 * 4 + b, v >> (8 * b));
                }
            }
        } else if (widen) {
            // lane L's pixel = bytes 3L .. 3L + 2 of the wave's 192: in the dwords of lanes 3L / 4 and the next one
            const uint32_t src = (3u * lane) >> 2, sh = (3u * lane) & 3u;
            const bool st = wave_px + lane < job.w;
            for (uint32_t k = 0; k < nrows; k++) {
                const uint32_t v = row_sum(k);
                const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src << 2), (int)v), hi = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((src + 1) << 2), (int)v);
                if (st) gstore_u32(row(k), (wave_px + lane) * 4, reorder(funnel(hi, lo, 8 * sh) | 0xFF000000u));
            }
        } else {
            // 4 -> 3 channels: the wave's 64 pixels are 48 dwords; lane L < 48 builds dword L = bytes 4L .. 4L + 3 of the 192
            // from the pixels 4L / 3 and the next one
            const uint32_t wpx = (cb * (kDecBlock / kWave) + wv) * kWave, nv = min((uint32_t)kWave, job.w - wpx); // (this wave's pixels: j4 = wpx + lane < w)
            const uint32_t p0 = (4u * lane) / 3u, r = 4u * lane - 3u * p0, have = 3u * nv; // bytes of the wave
            const uint32_t nb = lane < 48 ? (4u * lane + 4 <= have ? 4u : (4u * lane < have ? have - 4u * lane : 0u)) : 0u;
            const uint32_t off = wpx * 3 + 4u * lane;
            auto dword = [&](uint32_t acc) {
                const uint32_t a = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(p0 << 2), (int)acc), b = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(((p0 + 1) & 63u) << 2), (int)acc);
                return funnel((b & 0xFFFFFFu) >> 8, (a & 0xFFFFFFu) | (b << 24), 8 * r); // (b's 24 bits : a's 24 bits) >> 8 r
            };
            const bool ragged = __builtin_amdgcn_ballot_w64(nb - 1u < 3u) != 0; // the row ends inside some lane's dword (all lanes come along: they are the gather's sources)
            for (uint32_t k = 0; k < nrows; k++) {
                const uint32_t d = dword(reorder(row_sum(k)));
                if (nb == 4) gstore_u32(row(k), off, d);
                if (ragged && nb - 1u < 3u)
                    for (uint32_t q = 0; q < nb; q++) gstore_u8(row(k), off + q, d >> (8 * q));
            }
        }
        FPNG_TILE_STAMP(4);
    }
