// The text rewrites' tile loop (td_rewrite_common.h): the BODY of td_nfc_tiles<WRITE> and td_utf8_tiles<WRITE>, included inside the
// __global__ function itself, with `a` its arguments, WRITE its template parameter and P the pass's policy in scope.  A body and not a
// __device__ function template: __syncthreads_or / _and count the workgroup's waves from its size, and the compiler takes a launch's
// workgroups for whole ones (one scalar load of the size) only in code that stands in a __global__ function when it is first optimised.
// As an inlined function the same text costs every workgroup a compare and a dependent vector load at its start, which td_utf8_device
// on clean English paid with 2.3 % and td_nfc_device on English with 1.1 % (a workgroup a 4 KiB tile there).  No include guard: it is
// included once a kernel.
    __shared__ int32_t s_off[RC_LDS_DOCS];  // doc_off[kb + i] - t0, clamped to [RW_OFF_LO, RW_OFF_HI]
    __shared__ long long s_red[RW_THREADS / 64];
    const int tid = threadIdx.x;
    if (rewrite_bad_offsets(a, !WRITE)) return;
    if (WRITE && a.head[RW_H_FULL]) return;
    const int64_t total = a.doc_off[a.n_docs];
    const int shift = (int)(((uintptr_t)a.text) & 15);
    const int64_t ntiles = total > 0 ? (total + shift + RW_TILE - 1) / RW_TILE : 0;
    const auto off_of = [off = a.doc_off](int64_t d) { return off[d]; };
    typename P::Stats st = {};
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t t0 = t * RW_TILE - shift < 0 ? 0 : t * RW_TILE - shift;
        const int64_t s1 = (t + 1) * RW_TILE - shift < total ? (t + 1) * RW_TILE - shift : total;
        const int64_t b0 = t * RW_TILE + 16 * tid - shift, b = b0 < 0 ? 0 : b0, we = b0 + 16 < total ? b0 + 16 : total;
        const bool owns = b < we;
        bool fast = !owns, plain = !owns;
        if (owns) P::screen(a, b0, b, we, total, t * RW_THREADS + tid, fast, plain);
        // the tile's documents: kb the last that starts in front of t0 (t0 == 0: the first), its table, where a lane needs one
        const bool need = WRITE || !plain;
        int64_t kb = 0, nk = 0;
        bool lds = true;
        __syncthreads();  // (the tile before has read its table)
        if (__syncthreads_or(need)) {
            kb = t0 > 0 ? group_last_le(off_of, 0, a.n_docs, t0 - 1) : 0;
            nk = tile_table(s_off, off_of, kb, a.n_docs, t0, RW_OFF_LO, RW_OFF_HI, (int32_t)(s1 - t0), lds);
            if (!lds) nk = group_last_le(off_of, kb, a.n_docs, s1 - 1) - kb + 1;
            __syncthreads();
        }
        // ub(x), t0 - 1 <= x < s1: kb + the first entry of [0, nk] behind x (entry nk is at or behind s1)
        const auto ub_of = [&](auto rel) {
            return [=](int64_t x) {
                int64_t lo = 0, hi = nk;  // the answer lies in [lo, hi]
                const int64_t r = x - t0;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (rel(mid) > r) hi = mid;
                    else lo = mid + 1;
                }
                return kb + lo;
            };
        };
        const auto rel_lds = [&](int64_t i) { return (int64_t)s_off[i]; };
        const auto rel_glb = [&](int64_t i) { return a.doc_off[kb + i] - t0; };
        const auto lane = [&](auto mode, int64_t opos) {
            constexpr int MODE = decltype(mode)::value;
            if (!owns) return (int64_t)0;
            if (lds) return P::template lane<MODE>(a, b, we, total, ub_of(rel_lds), opos, st);
            return P::template lane<MODE>(a, b, we, total, ub_of(rel_glb), opos, st);
        };
        // a copied window: the output offsets of the documents that start in it
        const auto put_starts = [&](int64_t opos) {
            for (int64_t k = lds ? ub_of(rel_lds)(b - 1) : ub_of(rel_glb)(b - 1); k <= a.n_docs; ++k) {
                const int64_t s = a.doc_off[k];
                if (s >= we) break;
                a.out_doc_off[k] = opos + (s - b);
            }
        };
        if (!WRITE) {
            const int64_t n = !owns ? 0 : plain ? we - b : lane(std::integral_constant<int, RW_MEASURE>{}, 0);
            if (owns && plain) P::plain_window(st);
            const long long sum = block_sum(n, s_red);
            if (tid == 0) a.tile_base[t] = (unsigned long long)sum;
        } else {
            const int64_t n = !owns ? 0 : fast ? we - b : lane(std::integral_constant<int, RW_SIZE>{}, 0);
            long long sum;
            const int64_t opos = (int64_t)a.tile_base[t] + block_excl(n, s_red, sum);
            if (__syncthreads_and(fast)) {
                rewrite_group_copy(a.out + a.tile_base[t], a.text + t0, s1 - t0);
                if (owns) put_starts(opos);
            } else if (fast && owns) {
                for (int64_t q = b; q < we; ++q) a.out[opos + (q - b)] = a.text[q];
                put_starts(opos);
            } else {
                lane(std::integral_constant<int, RW_WRITE>{}, opos);
            }
        }
    }
    if (!WRITE) P::flush(a, st, s_red);
