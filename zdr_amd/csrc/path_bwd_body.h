// path_bwd_body.h — the body of the backward path kernels, included INSIDE k_path_bwd and k_path_bwd_emission (zdr_kernels.hip), which
// differ in their names and template parameter lists only: the including kernel provides SK, A, ENV, MT, EG and LG as template parameters
// or constants.  Text, not a function: k_path_bwd compiles to the very instructions it had when this was its body (tools/isa_diff.py).
    static_assert(!EG || (ENV && MT), "the environment gradient runs in the material-table environment kernels");
    static_assert(!LG || (MT && !EG), "the emission gradient runs in the material-table kernels, without the environment gradient");
    ZDR_KARGS_BEGIN
#define S (ka->S)
#define R (ka->R)
#define C (ka->C)
#define io (ka->io)
    extern __shared__ int lds[];        // BvhAccel: traversal stacks (sized at launch); unused otherwise
    __shared__ __attribute__((aligned(16))) float lds_q[ZDR_SCATTER_LDS_FLOATS];   // the queue writes g as one float4
    // The records of all paths of the wave share ONE pool of NS slots (80 bytes + a link each): a lane takes its home slot
    // (slot == lane) when that is free and otherwise the lowest free one, and gives the slot back when the sweep has read it.
    constexpr int NS = MT ? A::kPoolSlots - 2 : A::kPoolSlots;
    static_assert(NS >= 16 && NS <= 128, "the free mask is two 64-bit words");
    static_assert(ZDR_MAX_MATERIALS <= 256, "a material fits the upper byte of a link");
    typedef typename std::conditional<MT, unsigned short, unsigned char>::type link_t;
    __shared__ float4 lds_pool[5 * NS];                     // [float4 f][slot]
    __shared__ link_t lds_link[NS];                  // slot of the path's previous record (255: in scratch; a path's first record links to nothing and its link is never followed).  One byte: three more slots fit
    // bit s set: slot s is free.  The only state lanes share: lane 0 stores the mask after an allocation, the sweep's lanes OR freed
    // slots in, every lane reads it before the next allocation.  All three accesses are volatile or atomic and stand between
    // wavefront-scope fences, so the protocol does not rest on what the optimiser happens to do with plain LDS accesses.
    __shared__ __attribute__((aligned(16))) unsigned int lds_free[4];
    __shared__ int lds_origin[4];                           // first pixel of each item bank's tile
    float *lds_emit = nullptr;                              // LG: the wave's emission table (emit_add)
    if constexpr (LG) { __shared__ float lds_emit_table[3 * ZDR_EMIT_LDS_LIGHTS]; lds_emit = lds_emit_table; }
    const int lane = threadIdx.x;
    constexpr unsigned long long all_lo = (NS >= 64) ? ~0ull : ((1ull << (NS & 63)) - 1ull);
    constexpr unsigned long long all_hi = (NS > 64) ? ((NS >= 128) ? ~0ull : ((1ull << ((NS - 64) & 63)) - 1ull)) : 0ull;
    if (lane < 4) {
        const unsigned long long w = (lane < 2) ? all_lo : all_hi;
        lds_free[lane] = (unsigned int)((lane & 1) ? (w >> 32) : w);
    }
    __syncthreads();
    int last = -1;                                          // where the running path's most recent record lives: slot, 255 = scratch, -1 = none yet
    int deep_link[ZDR_MAX_RECORDED_DEPTH];
    Counters cnt;
    ItemBanks ib; ib.logical[0] = ib.logical[1] = -1; ib.inflight[0] = ib.inflight[1] = 0;
    int bank = 1;
    bool more_items = true;
    WorkItem w = decode_item(R, -1);
    uint32_t next_sample = 0, s_end = 0, perm_seed = 0;
    unsigned long long cam_mask = 0ull;
    f3 le_grad = mk3(0.0f);                                 // cotangent of the running path's pixel
    ScatterQueue q = MT ? scatter_queue_init_cells(lds_q, io.mt.ncells, R.cell_copies) : scatter_queue_init(lds_q, R.tex_h, R.tex_w, R.cell_copies);
    if constexpr (EG) q.lds_cells = nullptr;                // the map's cells are never in LDS (table_cell_env)
    if constexpr (LG) emit_table_init(lds_emit);
    PackedVertex deep[ZDR_MAX_RECORDED_DEPTH];
    int nrec = 0;
    PrimaryQueue pq = queue_init(io);
    f3 unused_sum = mk3(0.0f);
    bool alive = false; int pix = 0;
    PathState ps; Interaction it;
    ps.o = mk3(0.0f); ps.d = mk3(0.0f, 0.0f, 1.0f); ps.beta = mk3(1.0f); ps.L = mk3(0.0f); ps.pdf_bsdf = 1e30f; ps.depth = 0;
    ps.smp = sampler_make<SK>(C, 0, 0, 0, 0);
    it.p = mk3(0.0f); it.uv.x = 0.0f; it.uv.y = 0.0f; it.ns = mk3(0.0f, 0.0f, 1.0f); it.ng = it.ns; it.inst = 0; it.prim = 0;
    int stall = 0;
#ifdef ZDR_MEASURE_STATS
    unsigned long long st_trips = 0, st_shaded = 0, st_fin = 0, st_iters = 0, st_steps = 0;
#endif
    for (;;) {
        ZDR_KARGS_REFRESH
        bool progress = false;
        if (pq.tail - pq.head < (uint32_t)__popcll(__ballot(!alive))) {
            if (next_sample < s_end) {
                const uint32_t t0 = pq.tail;
                if constexpr (EG) {
                    // lane = pixel here: a camera ray that misses is a term of this lane's own pixel (weight 1 x mis of pdf_bsdf = 1e30)
                    auto camera_miss = [&](const EnvTerm &e) {
                        f3 g = mk3(0.0f);
                        if (w.valid && ((e.w.x != 0.0f) | (e.w.y != 0.0f) | (e.w.z != 0.0f))) g = e.w * pixel_cotangent(C, io, R.width, (uint32_t)w.x, (uint32_t)w.y);
                        env_push(q, io, R, g, e.uv);
                    };
                    primary_refill<SK, A, true, false, ENV, MT>(S, R, C, lds, w.x, w.y, w.valid, cam_mask, perm_seed, bank, next_sample, s_end, pq, unused_sum, cnt,
                                                                io.mt.inst_slot, camera_miss);
                } else if constexpr (LG) {
                    // lane = pixel here: a camera ray that ends on a light is a term of this lane's own pixel
                    auto camera_emit = [&](const EmitTerm &e) {
                        if (e.light >= 0) emit_add(lds_emit, io, S.light_count, e, pixel_cotangent(C, io, R.width, (uint32_t)w.x, (uint32_t)w.y));
                    };
                    primary_refill<SK, A, true, false, ENV, MT>(S, R, C, lds, w.x, w.y, w.valid, cam_mask, perm_seed, bank, next_sample, s_end, pq, unused_sum, cnt,
                                                                io.mt.inst_slot, NoEnvMiss(), camera_emit);
                } else
                primary_refill<SK, A, true, false, ENV, MT>(S, R, C, lds, w.x, w.y, w.valid, cam_mask, perm_seed, bank, next_sample, s_end, pq, unused_sum, cnt,
                                                            MT ? io.mt.inst_slot : nullptr);
                ib.inflight[bank] += pq.tail - t0;
                progress = true;
            } else if (more_items && ib.logical[bank ^ 1] < 0) {
                const int nxt = fetch_item(R, io.work_counters);
                if (nxt < 0) more_items = false;
                else {
                    bank ^= 1;
                    ib.logical[bank] = nxt;
                    w = decode_item(R, nxt);
                    perm_seed = (SK == 0) ? xxhash32_4((uint32_t)w.x, (uint32_t)w.y, C.seed, 0u) : 0u;
                    cam_mask = camera_mask(S, io, w);
                    if (lane == 0) { lds_origin[bank * 2] = w.x; lds_origin[bank * 2 + 1] = w.y; }
                    __syncthreads();
                    next_sample = w.s_begin; s_end = w.s_end;
                }
                stall = 0;
                continue;
            }
        }
        const int took = primary_pop<SK, MT>(S, C, !alive, nullptr, lds_origin, pq, ps, it, MT ? io.mt.inst_slot : nullptr);
        if (took >= 0) {
            {   // the pixel's cotangent / spp, straight from the image (load_le_grad; a popped path is inside the shard)
                const float4 gi = io.d_image[ps.smp.px + ps.smp.py * (uint32_t)R.width];
                if (C.spp_pow2) le_grad = mk3(gi.x * C.inv_spp, gi.y * C.inv_spp, gi.z * C.inv_spp);   // x / 2^k == x * 2^-k exactly: three IEEE divisions (~30 VALU per trip) less
                else { const float fs = (float)C.spp; le_grad = mk3(__fdiv_rn(gi.x, fs), __fdiv_rn(gi.y, fs), __fdiv_rn(gi.z, fs)); }
                if (any_nan(le_grad)) le_grad = mk3(0.0f);
            }
            nrec = 0;
            last = -1;
            alive = true; pix = took;
        }
        if (__ballot(alive) != 0ull) {
            progress = true;
            bool done = false;
            // sweep state: set when a path ends and used up before the trip is over — local to the trip, so that it
            // holds no registers while the vertex is shaded
            f3 term_Li = mk3(0.0f);
            PackedVertex plast;                             // the vertex shaded this trip, as recorded
            plast.a = plast.b = plast.c = plast.d = plast.e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            int pmat = 0;                                   // MT: material of plast
            int sw_k = -1;                                  // next vertex the sweep consumes
            bool want_store = false, mute = false;
            SweepState sw; sw.A = mk3(0.0f); sw.Lv = mk3(0.0f); sw.s = 0.0f; sw.Z = 0.0f; sw.tw = 0.0f;
            EnvTerm env_nee, env_miss;                      // EG: this trip's light sample on the environment, continuation ray that missed
            if constexpr (EG) { env_term_clear(env_nee); env_term_clear(env_miss); }
            if (alive) {
                PathVertex pv; float term_plfrac = 0.0f;
                Hit h;
                if (MT) pmat = it.mat;
                if constexpr (EG) done = path_shade<SK, A, true, false, ENV, MT, true>(S, R, C, io, lds, ps, it, pv, h, cnt, &env_nee);
                else if constexpr (LG) {
                    EmitTerm emit_nee;                      // (final when path_shade returns: added at once, nothing of it lives through the next ray)
                    done = path_shade<SK, A, true, false, ENV, MT, false, true>(S, R, C, io, lds, ps, it, pv, h, cnt, nullptr, &emit_nee);
                    emit_add(lds_emit, io, S.light_count, emit_nee, le_grad);
                } else
                done = path_shade<SK, A, true, false, ENV, MT>(S, R, C, io, lds, ps, it, pv, h, cnt);
                plast = pack_vertex(pv, le_grad, R.prb_mode);
                if constexpr (LG) {
                    if (!done) {
                        EmitTerm emit_hit; emit_term_clear(emit_hit);
                        path_continue<A, false>(S, lds, ps, h, cnt);
                        done = path_arrive<true, false, ENV, MT>(S, ps, h, it, term_Li, cnt, &term_plfrac, io.mt.inst_slot, nullptr, &emit_hit);
                        emit_add(lds_emit, io, S.light_count, emit_hit, le_grad);
                    }
                } else
                if constexpr (EG) {
                    if (!done) { path_continue<A, false>(S, lds, ps, h, cnt); done = path_arrive<true, false, ENV, MT>(S, ps, h, it, term_Li, cnt, &term_plfrac, io.mt.inst_slot, &env_miss); }
                } else
                if (!done) { path_continue<A, false>(S, lds, ps, h, cnt); done = path_arrive<true, false, ENV, MT>(S, ps, h, it, term_Li, cnt, &term_plfrac, MT ? io.mt.inst_slot : nullptr); }
                // Only a vertex whose path goes on is put away: when the path ends here (52 % of the vertices) the sweep below starts
                // from plast and nothing would read the record.  (5 LDS or scratch stores per vertex: 16.4 -> 15.5 ms for skipping
                // the vertices that stop at the shading step alone.)
                want_store = !done && ZDR_ABLATE != 3;      // (ablation 3, no sweep: nothing is kept, so no slot leaks)
                nrec++;
                if (done) {
                    alive = false;
                    // a NaN path (prb.py:100: contributes nothing) is swept all the same, muted: the sweep is what returns its slots
                    if (nrec > 0 && ZDR_ABLATE != 3) {
                        mute = any_nan(ps.L);
                        sw_k = nrec - 1;
                        sw.A = le_grad * term_Li; sw.Lv = sw.A; sw.s = 0.0f; sw.Z = 0.0f;
                        sw.tw = (R.prb_mode != ZDR_PRB_EXPECTATION) ? 0.0f : term_plfrac * dot(ps.beta, sw.A);   // emitter hit: d w_bsdf/dr = w_bsdf pl/(pb+pl) dln(pb)/dr
                    }
                }
            }
            // EG, reconverged: both terms are final (a NaN in one is dropped by its push, whatever the rest of the path does: env_push)
            if constexpr (EG) { env_push(q, io, R, env_nee.w * le_grad, env_nee.uv); env_push(q, io, R, env_miss.w * le_grad, env_miss.uv); }
            // Reconverged: hand out slots, all requests of the trip at once.  Home slot first (slot == lane: conflict-free LDS access);
            // the lanes whose home is taken — a path's second and later records, or a home another lane borrowed — are ranked, the free
            // slots are ranked (a lane speaks for slot `lane`, then for slot 64 + lane), and request r takes free slot r: one
            // ds_permute sends every free slot's number to the lane of its rank, one ds_bpermute lets a request read the number at
            // its own rank.  Slots above 63 go first so that homes stay free; no slot left: the record goes to scratch.
            {
                const unsigned long long req = __ballot(want_store);
                int slot = -1;
                if (req != 0ull) {
                    // acquire: the ds_or of the previous trips' sweeps (any lane) are visible to this read
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    const zdr_u4 fw = *(volatile const zdr_u4 *)lds_free;       // same address in every lane: a broadcast read
                    unsigned long long free_lo = ((unsigned long long)__builtin_amdgcn_readfirstlane(fw.y) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane(fw.x);
                    unsigned long long free_hi = ((unsigned long long)__builtin_amdgcn_readfirstlane(fw.w) << 32) | (unsigned int)__builtin_amdgcn_readfirstlane(fw.z);
                    const bool home = want_store && lane < NS && ((free_lo >> lane) & 1ull) != 0ull;
                    const unsigned long long took = __ballot(home);
                    free_lo &= ~took;
                    if (home) slot = lane;
                    const unsigned long long rest = req & ~took;
                    if (rest != 0ull && (free_lo | free_hi) != 0ull) {
                        const int nrest = __popcll(rest);
                        const int r = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(rest >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)rest, 0u));   // rank of this lane's request
                        const bool mine = want_store && !home;
                        const int cnt_hi = __popcll(free_hi), cnt_lo = __popcll(free_lo);
                        // free slots 64 + lane
                        const bool fh = ((free_hi >> lane) & 1ull) != 0ull;
                        const int jh = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(free_hi >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)free_hi, 0u));
                        const int at_hi = __builtin_amdgcn_ds_permute((fh ? jh : cnt_hi + (lane - jh)) << 2, lane);   // lane j < cnt_hi now holds the j-th free slot (minus 64)
                        const int pick_hi = __builtin_amdgcn_ds_bpermute(r << 2, at_hi);
                        if (mine && r < cnt_hi) slot = 64 + pick_hi;
                        free_hi &= ~__ballot(fh && jh < nrest);
                        // free slots `lane`, for the requests the upper slots did not serve
                        const int r2 = r - cnt_hi, nrest2 = nrest - cnt_hi;
                        const bool fl = ((free_lo >> lane) & 1ull) != 0ull;
                        const int jl = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(free_lo >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)free_lo, 0u));
                        const int at_lo = __builtin_amdgcn_ds_permute((fl ? jl : cnt_lo + (lane - jl)) << 2, lane);
                        const int pick_lo = __builtin_amdgcn_ds_bpermute((r2 & 63) << 2, at_lo);
                        if (mine && r2 >= 0 && r2 < cnt_lo) slot = pick_lo;
                        free_lo &= ~__ballot(fl && jl < nrest2);
                    }
                    if (lane == 0) {
                        const zdr_u4 nw = {(unsigned int)free_lo, (unsigned int)(free_lo >> 32), (unsigned int)free_hi, (unsigned int)(free_hi >> 32)};
                        *(volatile zdr_u4 *)lds_free = nw;
                    }
                    // release: the new mask is in LDS before any lane's ds_or of the sweep below (in-order LDS, one wave)
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                if (want_store) {
                    if (slot >= 0) {
                        float4 *r = lds_pool + slot;
                        r[0] = plast.a; r[NS] = plast.b; r[2 * NS] = plast.c; r[3 * NS] = plast.d; r[4 * NS] = plast.e;
                        lds_link[slot] = MT ? (link_t)((last & 255) | (pmat << 8)) : (link_t)last;
                        last = slot;
                    } else {
                        deep[nrec - 1] = plast; deep_link[nrec - 1] = MT ? ((last & 255) | (pmat << 8)) : last;
                        last = 255;
                    }
                }
            }
            ib.inflight[0] -= (uint32_t)__popcll(__ballot(done && (pix >> 6) == 0));
            ib.inflight[1] -= (uint32_t)__popcll(__ballot(done && (pix >> 6) == 1));
            // wave-uniform: sweep every finished path to its first vertex.  The sweep starts from the vertex packed this
            // trip (still in registers).
            PackedVertex cur = plast;
            int cur_mat = pmat;                             // MT: material of `cur`
            int loc = last;                                 // where the record of the sweep's next step lives
#ifdef ZDR_MEASURE_STATS   // measurement build (tools/bwd_stats.sh): how full are the trips and the sweep iterations
            st_trips++; st_shaded += (unsigned long long)__popcll(__ballot(alive || done));
            st_fin += (unsigned long long)__popcll(__ballot(sw_k >= 0));
#endif
            int sweep_cap = (ZDR_ABLATE == 4) ? 2 : ((ZDR_ABLATE == 5) ? 1 : 64);   // timing-only ablations 4 / 5: the sweep loop cut after 2 / 1 iterations
            // One step consumes `cur`, then fetches the record of the NEXT step into the same registers and only then queues the
            // gradient: the fetch (LDS, or scratch beyond the LDS records) is under way while the push runs, and no record is copied
            // (the loop runs 5.45 times per trip at 18 % of the lanes, profiles/r3_bwd_sweep_ablation.txt; fetching one step ahead
            // into a second register set cost 24 v_mov per iteration, and unrolling by two
            // with the sets swapping roles was slower still: profiles/r3_bwd_sweep_ablation.txt section 3).
            while (__ballot(sw_k >= 0) != 0ull && sweep_cap-- > 0) {
                const bool swp = sw_k >= 0;
#ifdef ZDR_MEASURE_STATS
                st_iters++; st_steps += (unsigned long long)__popcll(__ballot(swp));
#endif
                float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                f2 guv; guv.x = 0.0f; guv.y = 0.0f;
                const int gmat = cur_mat;
                if (swp) { g = sweep_vertex(cur, sw, guv, R.prb_mode); sw_k--; }
                // everything that reads `cur` is finished here, before the fetch below overwrites it (left alone the compiler sinks
                // part of the step below the fetch, loads into a second register set and copies — with a wait in front of the copies)
                asm volatile("" : "+v"(g.x), "+v"(g.y), "+v"(g.z), "+v"(g.w), "+v"(guv.x), "+v"(guv.y), "+v"(sw.A.x), "+v"(sw.A.y), "+v"(sw.A.z),
                             "+v"(sw.Lv.x), "+v"(sw.Lv.y), "+v"(sw.Lv.z), "+v"(sw.s), "+v"(sw.Z), "+v"(sw.tw) : : "memory");
                const bool fetch = swp && sw_k >= 0;
                const bool pooled = fetch && loc != 255;
                int nloc = -1;
                if (pooled) {
                    const float4 *r = lds_pool + loc;
                    cur.a = r[0]; cur.b = r[NS]; cur.c = r[2 * NS]; cur.d = r[3 * NS]; cur.e = r[4 * NS];
                    nloc = (int)lds_link[loc];
                    if (MT) { cur_mat = nloc >> 8; nloc &= 255; }
                }
                // LDS first: both kinds of fetch write the same registers (for different lanes), and the second kind waits for the
                // first to land — an LDS read is back in ~100 cycles, a scratch read in ~500 and behind the flush's atomics
                asm volatile("" ::: "memory");
                if (fetch && loc == 255) {
                    cur = deep[sw_k]; nloc = deep_link[sw_k];
                    if (MT) { cur_mat = nloc >> 8; nloc &= 255; }
                }
                // the slots just read are free again: a wavefront-scope RELEASE or, so the reads of the record above are ordered before it
                // (and this wave's LDS operations execute in order anyway: a later write cannot overtake the read)
                if (pooled) __hip_atomic_fetch_or(&lds_free[loc >> 5], 1u << (loc & 31), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WAVEFRONT);
                if (fetch) loc = nloc;
                scatter_push<MT, EG>(q, io.cells, swp && !mute && any_nonzero4(g) && !any_nan4(g), guv, g, R.tex_h, R.tex_w, ZDR_ABLATE, gmat, io.mt.m);   // prb.py:178-187
            }
        }
#pragma unroll
        for (int b = 0; b < 2; b++)                         // an item whose samples are all generated and whose paths have ended frees its bank
            if (ib.logical[b] >= 0 && ib.inflight[b] == 0 && (b != bank || next_sample >= s_end)) ib.logical[b] = -1;
        if (__ballot(alive) == 0ull && pq.tail == pq.head && next_sample >= s_end && !more_items) break;
        stall = progress ? 0 : stall + 1;
        if (stall > 4) { raise_device_error(S, ZDR_DEVERR_STALL); break; }   // cannot happen (every branch above makes progress); never spin on the GPU, never end silently
    }
    scatter_finish<MT, EG>(q, io.cells, R.tex_h, R.tex_w, ZDR_ABLATE, io.mt.m);
    if constexpr (LG) emit_table_finish(lds_emit, io, S.light_count);
    {   // every path has been swept, so every slot must be back: a leaked or doubly allocated slot is a protocol error, said aloud
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const zdr_u4 fw = *(volatile const zdr_u4 *)lds_free;
        const bool whole = fw.x == (unsigned int)all_lo && fw.y == (unsigned int)(all_lo >> 32) && fw.z == (unsigned int)all_hi && fw.w == (unsigned int)(all_hi >> 32);
        if (!whole && lane == 0 && stall <= 4 && ZDR_ABLATE == 0) raise_device_error(S, ZDR_DEVERR_POOL);
    }
#ifdef ZDR_MEASURE_STATS
    if (lane == 0) {
        atomicAdd(io.counters + 0, st_trips); atomicAdd(io.counters + 1, st_shaded); atomicAdd(io.counters + 2, st_fin);
        atomicAdd(io.counters + 3, st_iters); atomicAdd(io.counters + 4, st_steps);
        atomicAdd(io.counters + 5, q.st_flushes); atomicAdd(io.counters + 6, q.st_entries); atomicAdd(io.counters + 7, q.st_dups);
    }
#endif
#undef S
#undef R
#undef C
#undef io
