// Body of igemm_persistent_kernel / igemm_persistent_tiles_kernel / igemm_conv_tiles_kernel (conv_igemm.hip), included INSIDE each kernel definition: the text between
// the braces, written once.  The including kernel provides BM, BN, WM, WN, BF16, OUT_BF16, HAS_RES, SKIP, UPS, LIST as constants and
// a, mtiles, ntiles, M, tlist, tcount, tcap as values.  Not a device function that the two kernels call: that form (the halo kernel's)
// changed the register allocation of the dense instantiations -- 0 -> 44 B of scratch on the 196-channel 3 x 3 tile, 24 -> 64 B on the
// lateral -- while textual inclusion leaves each of them register for register where it was, under the name the profiles and the
// resource tests know.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef gim::Igemm<BM, BN, WM, WN, BF16, true> G;
    typedef Epilogue<G, OUT_BF16, HAS_RES, UPS, LIST> E;

    int nwalk = mtiles;   // M tiles this launch computes (LIST: mtiles = the patches of the map)
    if constexpr (LIST) {
        const int c = *tcount;
        nwalk = c < 0 ? 0 : (c < tcap ? c : tcap);
        nwalk = nwalk < mtiles ? nwalk : mtiles;
    }
    unsigned first, step, end;
    tile_list((unsigned)(nwalk * ntiles), first, step, end);   // (LIST: XCD-contiguous chunks of the ascending list -- neighbouring patches share upsample sources in one L2)
    if (first >= end) return;
    // LIST: walked tile index -> flat index of its patch's first pixel, through the list (clamped: an entry outside the map must not become
    // an address).  lw / lhgt: width / height of the output map (UPS: twice the upsample source's; else the 3 x 3 launch's own), tiles_x / per_img:
    // patches per map row / per image
    const int lw = LIST ? (UPS ? 2 * a.ups_w : a.Wo) : 0, lhgt = LIST ? (UPS ? 2 * a.ups_h : a.Ho) : 0;
    const int tiles_x = LIST ? lw / 32 : 1, per_img = LIST ? tiles_x * (lhgt / 8) : 1;
    auto list_entry = [&](const unsigned tile) -> int { return tlist[tile / (unsigned)ntiles]; };
    auto patch_row0 = [&](int e) -> int {
        e = e < 0 ? 0 : (e < mtiles ? e : mtiles - 1);
        const int b = e / per_img, r = e - b * per_img, ty = r / tiles_x, tx = r - ty * tiles_x;
        return (b * lhgt + ty * 8) * lw + tx * 32;
    };
    const gim::MainloopArgs ml = mainloop_args(a, M, G::ES);
    const int nkt = a.kpad * G::ES / KTB;

    E epi;
    if constexpr (!BF16) { if (a.split16) epi.wscale = 4096.f; }
    GIM_TT(conv, epi.wave, 0);
    unsigned long long tt_k = 0, tt_e = 0, tt_n = 0, tt_a = 0, tt_b = 0;   // GIM_TIMING: K-loop / epilogue totals over this workgroup's tiles
    (void)tt_k; (void)tt_e; (void)tt_n; (void)tt_a; (void)tt_b;
    G g, gn;  // staging coordinates of the current / the next tile
    typename G::Acc acc;
    typename E::Res rres;
    int buf = 0;
    int m0 = (int)(first / ntiles) * BM, n0 = (int)(first % ntiles) * BN;
    int le_n = 0;   // LIST: the list entry of the NEXT tile, fetched one tile ahead of the decode in front of the cross-tile prefetch
    if constexpr (LIST) {
        m0 = patch_row0(list_entry(first));
        if (first + step < end) le_n = list_entry(first + step);
    }
    epi.init_acc(a, acc, n0);
    if constexpr (LIST) g.template decode_patch<!UPS>(ml, m0, lw, n0);
    else g.decode(ml, m0, n0);
    g.stage_issue(ml, smem, 0, 0, a.ktab[G::ktab_index(0)]);
    int e_nxt = a.ktab[G::ktab_index(nkt > 1 ? 1 : 0)];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    for (unsigned tile = first; tile < end; tile += step) {
        const unsigned tile_n = tile + step;
        const bool has_next = tile_n < end;
        int m0n = (int)(tile_n / ntiles) * BM;
        const int n0n = (int)(tile_n % ntiles) * BN;
        if constexpr (LIST) {
            m0n = has_next ? patch_row0(le_n) : m0;
            if (tile_n + step < end) le_n = list_entry(tile_n + step);   // consumed at the top of the next tile: a whole K loop away
            if (has_next) gn.template decode_patch<!UPS>(ml, m0n, lw, n0n);
        } else {
            if (has_next) gn.decode(ml, m0n, n0n);
        }
        tt_a = GIM_TT_NOW();
        // ---- K loop: only MFMAs touch the accumulators in here ------------------------------------------
        auto kloop = [&](auto live, auto split16) __attribute__((always_inline)) {
            for (int kt = 0; kt < nkt; ++kt) {
                const bool last = kt + 1 == nkt;
                int k2 = kt + 2;
                if (k2 >= nkt) k2 -= nkt;
                if (k2 >= nkt) k2 = 0;  // nkt == 1
                const int e_n2 = a.ktab[G::ktab_index(k2)];
                if (!last) g.stage_issue(ml, smem, buf ^ 1, kt + 1, e_nxt);
                else if (has_next) gn.stage_issue(ml, smem, buf ^ 1, 0, e_nxt);  // first slab of the next tile
                if (last) epi.prefetch_res(a, rres, m0, n0, M);
                if constexpr (decltype(split16)::value != 0) G::template compute_split16<decltype(live)::value>(smem, buf, acc, epi.wscale);
                else G::template compute<decltype(live)::value>(smem, buf, acc);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                buf ^= 1;
                e_nxt = e_n2;
            }
        };
        if constexpr (SKIP && G::TN > 1) {
            // the wave's last channel fragment holds only padding channels (wave-uniform)
            if (n0 + epi.wn * G::WTN + (G::TN - 1) * 32 >= a.N) kloop(IntC<G::TN - 1>(), IntC<BF16 ? 0 : 1>());   // (fp32 operands reach this tile as split launches only: dispatch_persistent checks a.split16 on both branches)
            else kloop(IntC<G::TN>(), IntC<BF16 ? 0 : 1>());
        } else if constexpr (!BF16) {
            if constexpr (BM == 256 && BN == 256) kloop(IntC<G::TN>(), IntC<1>());   // (only split launches are sent to this tile: dispatch_persistent checks a.split16 on both branches)
            else if (a.split16) kloop(IntC<G::TN>(), IntC<1>());   // (a second copy of the loop, selected per launch)
            else kloop(IntC<G::TN>(), IntC<0>());
        } else {
            kloop(IntC<G::TN>(), IntC<0>());
        }
        tt_b = GIM_TT_NOW(); tt_k += tt_b - tt_a;
        epi.run(a, acc, rres, smem + (buf ^ 1) * G::STAGE, m0, n0, M, smem + 2 * G::STAGE);  // buf ^ 1: the stage just consumed; UPS: patch rows behind the stages
        epi.init_acc(a, acc, n0n < a.npad ? n0n : 0);
        g = gn;
        m0 = m0n; n0 = n0n;
        __syncthreads();  // the transposition tile lives in a stage buffer the next slab's DMA will overwrite
        tt_e += GIM_TT_NOW() - tt_b; ++tt_n;
    }
    GIM_TT(conv, epi.wave, 1);
    GIM_TT_SET(conv, epi.wave, 4, tt_k); GIM_TT_SET(conv, epi.wave, 5, tt_e); GIM_TT_SET(conv, epi.wave, 6, tt_n);
