// tdlo_estep_body.inc -- the E-step's statements (trackdlo.cpp:278-389), included into the body of a kernel (see tdlo_estep_body.h).  The including scope provides:
//   template parameters / constants   T, NCH, VIS, EB, SINGLE  and  constexpr bool FUSED
//   const FrameDev &f;  char smem[] (the dynamic LDS);  const EstepHand<T> *hand  (FUSED: what the M-step half hands over; otherwise nullptr)
//   (an EstepHand<T, true>: the kernel has zeroed the wave's accumulators and stands behind a barrier with nothing written to LDS since -- FRONT below)
// The statements `return` from the including kernel, so they come last in it.  What the E-step computes and what bounds it: the head of tdlo_device.hip.
    constexpr int NWE = EB / 64;
    constexpr bool FRONT = std::remove_cv_t<std::remove_pointer_t<decltype(hand)>>::kFront;
#ifdef TDLO_ESTEP_STAMPS
    if (threadIdx.x == 0) atomicMin(&f.dbg[32], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
#ifdef TDLO_ESTEP_STAMPS
#define ESTAMP(i) do { if (threadIdx.x == 0 && blockIdx.x == 0) f.dbg[40 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define ESTAMP(i) do { } while (0)
#endif
    // -DTDLO_ESTEP_PHASES: shader clocks per phase, summed over the batches of wave 0 of the middle workgroup (scripts/gpu_ephases.py)
#ifdef TDLO_ESTEP_PHASES
    unsigned long long ph_prev = __builtin_amdgcn_s_memtime(), ph_acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define EPHASE(i) do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); const unsigned long long t_ = __builtin_amdgcn_s_memtime(); ph_acc[i] += t_ - ph_prev; ph_prev = t_; } while (0)
#else
#define EPHASE(i) do { } while (0)
#endif
    ESTAMP(0);
    const auto stg = TDLO_AS_GLOBAL(IterState, f.st);
#ifdef TDLO_TIMELINE      // wall-clock (100 MHz) begin of the first workgroup / end of the last one, iterations 20..27 (scripts/gpu_timeline.py)
    const int tl_it = stg->it - 20;
    if (threadIdx.x == 0 && blockIdx.x == 0 && tl_it >= 0 && tl_it < 8) f.dbg[4 * tl_it] = __builtin_amdgcn_s_memrealtime();
#endif
    const int M = f.M;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // tile rows: one frame (SINGLE) of up to 64 nodes cannot fill the GPU anyway, so it keeps the whole window in the tile; batches use the
    // small tile (two workgroups per CU) and recompute the memberships of the later chunks of a wide window.  Chains beyond 64 nodes use the
    // small tile as well: their windows are far wider than any tile (most chunks are recomputed either way), and the 64-row tile of an
    // fp64 workgroup is 133 KB -- one workgroup per CU, one wave per SIMD, every dependent instruction a stall
    constexpr int TR = tile_rows<T>(NCH);
    constexpr int RT = (NCH == 1 && SINGLE) ? kChunk : TR;
    constexpr int RS = (RT / TR) * TR;                     // stored rows: whole chunks only
    const int rows = M < RT ? M : RT;
    // LDS carve (every offset a multiple of 16 bytes).  FRONT: taken from estep_carve (tdlo_estep_body.h), the definition the kernel zeroed the accumulators by --
    // the same expressions; as one shared definition for every instantiation they came out of the compiler as different code for k_estep and k_iter_fused
    V4<T> *nodesL = (V4<T> *)smem;                                    // M
    V4<T> *pts = FRONT ? estep_carve<T, NWE>(smem, M, rows).pts : nodesL + M;                                          // NWE x kPtsStride: point i of a wave at i + (i >> 4), see the column sums
    T *lvL = FRONT ? estep_carve<T, NWE>(smem, M, rows).lvL : (T *)(pts + NWE * kPtsStride);                           // M rounded up to 4
    T *pbase = FRONT ? estep_carve<T, NWE>(smem, M, rows).pbase : lvL + ((M + 3) & ~3);
    T *pb = pbase + (size_t)wave * rows * kPStride;
    double *scratch = FRONT ? estep_carve<T, NWE>(smem, M, rows).scratch : (double *)(pbase + (((size_t)NWE * rows * kPStride + 7) & ~(size_t)3));   // 16-byte aligned, stays an LDS pointer

    const auto nodes = TDLO_AS_CONST(V4<T>, f.nodes);
    const auto xs = TDLO_AS_GLOBAL(T, f.Xs);
    const size_t ld = f.ldx;
    // first wave of loads: this wave's first points, iteration state, nodes for the LDS copy
    const int batch0 = blockIdx.x * NWE + wave;
    T x = 0, y = 0, z = 0;
    if constexpr (FUSED) { x = hand->x; y = hand->y; z = hand->z; }          // (requested at the top of the launch, in front of the M-step half)
    else {
        const int n = batch0 * 64 + lane;
        if (n < f.N0) { x = xs[n]; y = xs[ld + n]; z = xs[2 * ld + n]; }     // N <= N0: always in bounds
    }
    // ---- EVERYTHING this kernel reads from memory before its first barrier is requested here, back to back, in ONE round trip with the points above: the
    // iteration state, this thread's node for the LDS copy, this lane's node.  (Until round 6 the state's `done` was waited for on its own -- the branch below
    // needs it -- then N, k2, c_norm were requested, waited for, then the nodes: three round trips in a row, and the boost, the window radius and the parity
    // one more each behind the barrier: 3 500 clocks of a 8 000-clock workgroup at C2 spent waiting for memory, scripts/archive/gpu_estamps.py + the ISA.)
    // (fp32 only: the fp64 instantiations -- two waves per SIMD, registers full, chains of hundreds of nodes -- measured 0.4 % ... 4 % SLOWER with the requests up
    //  front and their values held across the kernel; they keep the order of before)
    constexpr bool EARLY = sizeof(T) == 4;
    // FUSED: nothing of this comes from memory -- the M-step half of the launch has left the state in LDS (hand->st) and the nodes in nodesL, behind a barrier;
    // it has looked at `done` itself, and the accumulator buffer is the launch's (hand->acc_buf)
    static_assert(!FUSED || (sizeof(T) == 4 && NCH == 1 && SINGLE && !VIS), "the one-launch iteration carries the fp32 E-step of one frame on up to 64 nodes");
    const int done = FUSED ? 0 : stg->done;
    const int it0 = FUSED ? 0 : (EARLY ? stg->it : 0);
    int N; T k2, cn;
    if constexpr (FUSED) { N = hand->st->N; k2 = (T)hand->st->k2; cn = (T)hand->st->c_norm; }
    else if constexpr (EARLY) { N = stg->N; k2 = (T)stg->k2; cn = (T)stg->c_norm; }
    const int shb_e = FRONT ? 0 : (FUSED ? hand->st->sh_boost : (EARLY ? stg->sh_boost : 0));     // (FRONT: fp32 mode, where the M-step half sets 0 by construction)
    const double rwin_e = FUSED ? hand->st->rwin32 : (EARLY ? stg->rwin32 : 0.0);
    const int par_e = FUSED ? hand->acc_buf : (it0 & 1);
    const auto qg = TDLO_AS_GLOBAL(V4<T>, f.nodes);
    V4<T> nd0; nd0.x = 0; nd0.y = 0; nd0.z = 0; nd0.w = 0;
    if (!FUSED && EARLY && tid < M) { nd0.x = qg[tid].x; nd0.y = qg[tid].y; nd0.z = qg[tid].z; nd0.w = qg[tid].w; }
    // One frame that cannot fill the GPU, chains of up to 64 nodes (round 6): the kernel is a chain of latencies there (one wave per SIMD: 8 500 clocks per batch, of
    // which the scalar node loads of the two node loops and the LDS reads of the range tests are round trips nothing overlaps).  Lane l keeps node l in registers for the
    // whole kernel and a node's values reach the wave by v_readlane -- the same values in the same operand positions (an SGPR either way): the same bits, no round trip.
#ifdef TDLO_NO_LANE_NODES          // (scripts/build_variant.sh nolane -DTDLO_NO_LANE_NODES: the comparator of scripts/gpu_ab.sh)
    constexpr bool LANE_NODES = false;
#else
    constexpr bool LANE_NODES = SINGLE && NCH == 1;
#endif
    V4<T> qn; qn.x = 0; qn.y = 0; qn.z = 0; qn.w = 0;
    if constexpr (FUSED) { if (LANE_NODES && lane < M) qn = nodesL[lane]; }
    else
    if (LANE_NODES && lane < M) { qn.x = qg[lane].x; qn.y = qg[lane].y; qn.z = qg[lane].z; qn.w = qg[lane].w; }
    if (!FUSED && SINGLE && f.late_aJ != nullptr && f.late_mstep == 0 && blockIdx.x == 0 && (EARLY ? it0 : stg->it) == 0) {
        // (tracking_step's second registration) the priors the host formed while the set-up kernel ran: to their place in the node block, for the
        // M-step of this and every later iteration
        double *dj = (double *)f.aJ, *dy = (double *)f.aYd;
        for (int i = threadIdx.x; i < f.M; i += EB) dj[i] = f.late_aJ[i];
        for (int i = threadIdx.x; i < 3 * f.M; i += EB) dy[i] = f.late_aYd[i];
    }
    if constexpr (FUSED) {
    } else if constexpr (EARLY) {
        if (tid < M) nodesL[tid] = nd0;
        for (int m = tid + EB; m < M; m += EB) { V4<T> o; o.x = qg[m].x; o.y = qg[m].y; o.z = qg[m].z; o.w = qg[m].w; nodesL[m] = o; }
    } else {
        N = stg->N; k2 = (T)stg->k2; cn = (T)stg->c_norm;
        for (int m = tid; m < M; m += EB) { V4<T> o; o.x = qg[m].x; o.y = qg[m].y; o.z = qg[m].z; o.w = qg[m].w; nodesL[m] = o; }
    }
    auto lane_val = [&](T v, int src) -> T {          // v of lane src (wave-uniform), as a wave-uniform operand
        if constexpr (sizeof(T) == 4) return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(v), src));
        else return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
    };
    if (done) return;
    double lv_span = 0;      // VIS: the largest -log2 v_m + log2 v_m' over the nodes -- how far the visibility weights can lower a nearest node's membership against another's
    if (VIS) {
        // P_vis rows, :362-372: v_m = exp(-k_vis * dmin_m) / sum, folded into the exponent as log2 v_m
        double tot = 0, dmx = 0, dmn = 1e300;
        for (int m = tid; m < M; m += EB) {
            double d = ::sqrt(Num<T>::from_bits(f.dminbits[m]));
            if (d > 10000.0) d = 10000.0;                        // initial value of :282
            if (d <= f.vis_thr) d = 0;                           // :291-293
            tot += ::exp(-f.k_vis * d);
            dmx = d > dmx ? d : dmx; dmn = d < dmn ? d : dmn;
        }
        tot = block_sum_n<NWE>(tot, scratch);
        {   // (max and min of d over the nodes: a wave reduction each, the waves through the same scratch)
            dmx = wave_max_nonneg(dmx); dmn = wave_min_nonneg(dmn);
            __syncthreads();
            if (lane == 0) { scratch[wave] = dmx; scratch[NWE + wave] = dmn; }
            __syncthreads();
#pragma unroll
            for (int w_ = 0; w_ < NWE; ++w_) { dmx = scratch[w_] > dmx ? scratch[w_] : dmx; dmn = scratch[NWE + w_] < dmn ? scratch[NWE + w_] : dmn; }
            lv_span = f.k_vis * (dmx - dmn) * 1.4426950408889634;
            if (!(lv_span > 0)) lv_span = 0;
        }
        for (int m = tid; m < M; m += EB) {
            double d = ::sqrt(Num<T>::from_bits(f.dminbits[m]));
            if (d > 10000.0) d = 10000.0;
            if (d <= f.vis_thr) d = 0;
            lvL[m] = (T)(-f.k_vis * d * 1.4426950408889634 - ::log2(tot));
        }
    }
    if constexpr (!FRONT) __syncthreads();
    ESTAMP(1);
    EPHASE(0);

    // running sums in 64-bit fixed point (acc_fix at the grain of one wave x one batch; integer from there on: tdlo_devcommon.h)
    long long accQ = 0;
    const int shb = EARLY ? shb_e : stg->sh_boost;         // (fp64 mode: extra digits for R, twice as many for Q, while sigma is small: set_iter_consts)
    const double scP = acc_scale(f.acc_sh[0]), scR = acc_scale(f.acc_sh[1] + shb), scQ = acc_scale(f.acc_sh[2] + 2 * shb);
    // every converted value is checked against its limit (FrameDev::acc_lim: exact conversion, no wrap-around of the totals; a NaN fails
    // the comparison too): one compare per conversion into a lane mask, looked at once per wave at the end
    const double limP = f.acc_lim[0], limR = f.acc_lim[1] * acc_scale(-shb), limQ = f.acc_lim[2] * acc_scale(-2 * shb);
    // (a node's share of Q -- the column sums' tail -- is one conversion for up to a batch's points: held to the conversion's own exactness bound, 2^51 units)
    const double limQn = acc_scale(51 - (f.acc_sh[2] + 2 * shb));
    bool acc_ok = true;
    // NCH == 1 (M <= 64): windowed variant.  The cloud is sorted by nearest node, so the 64 points of a
    // wave sit on a short piece of the chain, and every membership whose exponent is below -151 (fp32;
    // -1080 in fp64) is EXACTLY zero: only the nodes inside an arc-length window around the wave's
    // nearest-pair range can contribute, the others are skipped -- same sums, bit for bit.
    // [M][4] 64-bit accumulators in LDS (ds_add_u64 without return: integer sums, so neither the order nor who adds matters).  Up to 64 nodes: one set
    // per wave (no contention, 1.6 KB each at M = 50).  Longer chains: ONE set per workgroup -- per-lane register accumulators (4 x NCH 64-bit values
    // and a cross-lane gather per chunk) had held the fp64 kernel at 227 VGPRs, and a set per wave would cost the second workgroup of a CU its LDS
    long long *accL = FRONT ? estep_accL(scratch, M, wave, true) : (long long *)(scratch + 16) + (NCH == 1 ? (size_t)wave * M * 4 : (size_t)0);
    if (NCH == 1) {
        if constexpr (!FRONT) for (int i = lane; i < M * 4; i += 64) accL[i] = 0;
    } else {
        for (int i = tid; i < M * 4; i += EB) accL[i] = 0;
        __syncthreads();
    }
    // Node window: E / |k2| (a squared arc length, left by the M-step; E bits: FrameDev::win_e32 / win_e64), widened by what the visibility
    // weights can take from a nearest node's membership.  A wave leaves node m out when (coord distance to the wave's nearest pairs)^2 exceeds
    // (largest nearest-node distance of the wave)^2 + this: every point's membership of m is then below 2^-E of its largest one
    const T R2win = (T)((EARLY ? rwin_e : stg->rwin64) * (1.0 + (VIS ? lv_span / (sizeof(T) == 4 ? f.win_e32 : f.win_e64) : 0.0)));

    const int nbatch = (N + 63) >> 6;
    for (int batch = batch0; batch < nbatch; batch += f.nblkE * NWE) {
        const int n = batch * 64 + lane;
        const bool valid = n < N;
        EPHASE(6);
        if (batch != batch0) { x = 0; y = 0; z = 0; if (valid) { x = xs[n]; y = xs[ld + n]; z = xs[2 * ld + n]; } }
        else if (!valid) { x = 0; y = 0; z = 0; }     // the speculative first load may have read past the kept points
        EPHASE(1);
        // ---- nearest node: argmax of the Euclidean membership (:298-310) == argmin of d2, first index
        // The cloud is sorted by nearest node, so the wave's points sit in a small ball (centre = lane 0's point, radius
        // rw).  With D_m = |y_m - centre|: every point is within min_m D_m + rw of some node and at least D_m - rw away
        // from node m, so node m can be the nearest node of a point of this wave only if D_m <= min D + 2 rw.  The search
        // runs over the index range of those candidates (a relative margin of 1e-4 dwarfs the rounding of the fp32
        // distances): the same argmin, first index on ties, from typically 5 instead of M candidates.
        int plo = 0, phi = M - 1;
        {
            const T cx = bcast_first(x), cy = bcast_first(y), cz = bcast_first(z);      // all 64 lanes are active here
            T r2 = valid ? (x - cx) * (x - cx) + (y - cy) * (y - cy) + (z - cz) * (z - cz) : T(0);
            // (the test runs on the SQUARES: D_m^2 <= lim^2 -- one square root per wave after the reduction instead of one per lane and chunk, 5 x ~25
            //  fp64 instructions per batch at 300 nodes; the margin covers the rounding of the square as it covers that of the distances)
            T Dm[NCH];
            T dmin_w = Num<T>::inf();
#pragma unroll
            for (int c = 0; c < NCH; ++c) {                  // lane = node 64 c + lane
                const int m = c * kChunk + lane;
                Dm[c] = Num<T>::inf();
                if (m < M) { const V4<T> qq = LANE_NODES ? qn : nodesL[m]; Dm[c] = (qq.x - cx) * (qq.x - cx) + (qq.y - cy) * (qq.y - cy) + (qq.z - cz) * (qq.z - cz); }
                dmin_w = tmin(dmin_w, Dm[c]);
            }
            wave_max_min_nonneg(r2, dmin_w, r2, dmin_w);          // (both reductions in one folded butterfly)
            T lim = (Num<T>::sqrt_fast(dmin_w) + T(2) * Num<T>::sqrt_fast(r2)) * T(1.0001) + T(1e-30);
            lim = lim * lim;
            int first = M, last = -1;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const unsigned long long cand = __ballot(c * kChunk + lane < M && Dm[c] <= lim);
                if (cand) {
                    const int lo_c = c * kChunk + (int)__builtin_ctzll(cand), hi_c = c * kChunk + 63 - (int)__builtin_clzll(cand);
                    first = lo_c < first ? lo_c : first; last = hi_c > last ? hi_c : last;
                }
            }
            if (last >= 0) { plo = first; phi = last; }
            plo = __builtin_amdgcn_readfirstlane(plo); phi = __builtin_amdgcn_readfirstlane(phi);
        }
        ESTAMP(8);      // (instrumented builds: the candidate range is known; the rest of the phase is the candidates' loop)
        T best = Num<T>::inf();
        int a = plo;
        // candidates in groups of 4: the group's scalar loads are issued together (index clamped to phi), the evaluations
        // beyond phi are skipped by wave-uniform branches -- one scalar-memory latency per group instead of one per node
        if constexpr (LANE_NODES) {
            for (int m = plo; m <= phi; ++m) {           // (the candidate's coordinates from its lane: nothing to wait for)
                const T dx = x - lane_val(qn.x, m), dy = y - lane_val(qn.y, m), dz = z - lane_val(qn.z, m);
                const T d2 = dx * dx + dy * dy + dz * dz;
                if (d2 < best) { best = d2; a = m; }
            }
        } else {
            int m0 = plo;
            for (; m0 + 3 <= phi; m0 += 4) {             // whole groups: ONE scalar load of four nodes, no per-node index clamp or test
                const Node4<T> q4 = load_node4<T>(f.nodes, m0);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const T dx = x - q4.v[4 * k], dy = y - q4.v[4 * k + 1], dz = z - q4.v[4 * k + 2];
                    const T d2 = dx * dx + dy * dy + dz * dz;
                    if (d2 < best) { best = d2; a = m0 + k; }
                }
            }
            if (m0 <= phi) {                             // the last, partial group: the same load (entries behind the last node stay inside
                const Node4<T> q4 = load_node4<T>(f.nodes, m0);          // the slot's node block), evaluations beyond phi skipped wave-uniformly
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (m0 + k <= phi) {
                        const T dx = x - q4.v[4 * k], dy = y - q4.v[4 * k + 1], dz = z - q4.v[4 * k + 2];
                        const T d2 = dx * dx + dy * dy + dz * dz;
                        if (d2 < best) { best = d2; a = m0 + k; }
                    }
                }
            }
        }
        // The reference takes the nearest node as the argmax of exp(-d2 / (2 sigma2)) / (column sum + c) (:298-310).  When even the nearest
        // node's exponent is below -1075 in base 2 every entry of the column has underflowed to exactly zero in fp64, and the argmax of an
        // all-zero column is its FIRST index: node 0 (from there the end-node rule of :313-321 can give node 1 a membership of exp(0) = 1 for a
        // point a metre away -- the reference's behaviour, reproduced).  Reachable once sigma is below d / 38.6 for a kept point d <= 0.1 m
        // from the chain, i.e. sigma2 < 6.7e-6: rare, so the wave looks at it together.
        {
            const bool under = best * k2 < T(-1075);          // (lanes without a point: whatever they decide is masked out below, as their nearest node is)
            if (__builtin_expect(__ballot(under) != 0ull, 0)) {
                const V4<T> q0 = nodesL[0];
                const T dx0 = x - q0.x, dy0 = y - q0.y, dz0 = z - q0.z;
                const T d0 = dx0 * dx0 + dy0 * dy0 + dz0 * dz0;
                if (under) { a = 0; best = d0; }
            }
        }
        ESTAMP(2);
        EPHASE(2);
        // ---- second node by distance (:313-329)
        const int c1 = (a == 0) ? 2 : a - 1;
        const int c2 = (a == M - 1) ? M - 3 : a + 1;
        const V4<T> q1 = nodesL[c1], q2 = nodesL[c2], qa = nodesL[a];
        T dx = x - q1.x, dy = y - q1.y, dz = z - q1.z;
        const T s1 = dx * dx + dy * dy + dz * dz;
        dx = x - q2.x; dy = y - q2.y; dz = z - q2.z;
        const T s2 = dx * dx + dy * dy + dz * dz;
        bool first; T eb;
        if constexpr (sizeof(T) == 4) { first = s1 < s2; eb = Num<T>::sqrt_fast(first ? s1 : s2); }      // the decision of :324 on the squares: one square root
        else { const T e1 = Num<T>::sqrt_fast(s1), e2 = Num<T>::sqrt_fast(s2); first = e1 < e2; eb = first ? e1 : e2; }   // fp64: the reference's comparison of norms
        const int b = first ? c1 : c2;
        const T cb = first ? q1.w : q2.w;
        const T ea = Num<T>::sqrt_fast(best);
        const bool a_lo = a < b;
        const int lo = a_lo ? a : b, hi = a_lo ? b : a;
        const T d_lo = a_lo ? ea : eb, d_hi = a_lo ? eb : ea;
        const T c_lo = a_lo ? qa.w : cb, c_hi = a_lo ? cb : qa.w;

        // ---- node window of this wave
        int wlo = 0, whi = M - 1;
        // fp64 (round 6): the range of the nearest pairs' INDICES and "some point has the end-node gap" go through one folded butterfly of 32-bit keys
        // (the coordinates of the range's ends are looked up: coord is non-decreasing) instead of two more fp64 wave reductions, and they let the
        // membership loop take the nodes below every point's lo / above every point's hi without a per-point decision (k_estep2's scheme)
        int min_lo = 0, max_hi = M - 1;
        bool gap_any = true;
        {
            T amin, amax, bmx;                                                                                          // coord >= 0
            if constexpr (sizeof(T) == 8) {
                const unsigned klo = valid ? (unsigned)(kMaxNodes - lo) : 0u, khi = valid ? (unsigned)hi : 0u, kgap = (valid && hi - lo != 1) ? 1u : 0u;
                const unsigned zz = rows_max_u32(fold16_max(fold32_max(klo, khi), fold32_max(kgap, kgap)));
                min_lo = kMaxNodes - __builtin_amdgcn_readlane((int)zz, 15); max_hi = __builtin_amdgcn_readlane((int)zz, 47);
                gap_any = __builtin_amdgcn_readlane((int)zz, 31) != 0;
                bmx = wave_max_nonneg(valid ? best : T(0));
                amin = nodesL[min_lo].w; amax = nodesL[max_hi].w;
            } else {
                wave_min_max_max_nonneg(valid ? c_lo : Num<T>::inf(), valid ? c_hi : T(0), valid ? best : T(0), amin, amax, bmx);   // (three reductions, one folded butterfly)
            }
            const T Rwin = Num<T>::sqrt_fast(bmx + R2win);
            int first = M, last = -1;
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const int m = c * kChunk + lane;
                const T cm = (m < M) ? (LANE_NODES ? qn.w : nodesL[m].w) : Num<T>::inf();
                const unsigned long long inw = __ballot(m < M && cm > amin - Rwin && cm < amax + Rwin);
                if (inw) {
                    const int lo_c = c * kChunk + (int)__builtin_ctzll(inw), hi_c = c * kChunk + 63 - (int)__builtin_clzll(inw);
                    first = lo_c < first ? lo_c : first; last = hi_c > last ? hi_c : last;
                }
            }
            if (last >= 0) { wlo = first; whi = last; }
            wlo = __builtin_amdgcn_readfirstlane(wlo); whi = __builtin_amdgcn_readfirstlane(whi);
        }

        ESTAMP(3);
        EPHASE(3);
        // ---- unnormalised membership, column sum, Q (:354-383)
        // adj: no point of this wave has the end-node gap (hi == lo + 2), the cheaper form of the exponent applies
        const bool adj = sizeof(T) == 8 ? !gap_any : __ballot(valid && hi - lo != 1) == 0;
        // fp64, chains beyond 64 nodes, a window too wide for the tile (C5's first iterations: the whole chain): lane = node for this batch (tdlo_estep_wide.h)
        if constexpr (sizeof(T) == 8 && NCH > 1) {
            constexpr int WCH = NCH < 5 ? NCH : 5;
            if (whi - wlo + 1 >= f.estep_wide_min && whi - wlo + 1 <= 64 * WCH) {
                estep_wide_batch<WCH, VIS>(lane, wlo, whi, batch * 64, N, adj, min_lo, max_hi, x, y, z, lo, hi, c_lo, d_lo, c_hi, d_hi, k2, cn, nodesL, lvL, (double *)pb, accL,
                                           scP, scR, scQ, limP, limR, limQ, limQn, accQ, acc_ok);
                EPHASE(5);
                continue;
            }
        }
        T sum = 0, qs = 0;
        // fp64: the argument of the exponent without a per-point decision for the nodes at or below every point's lo (m <= min_lo) and at or above
        // every point's hi (m >= max_hi) -- wave-uniform branches; the per-point form in between (and everywhere when a pair has the end-node gap)
        auto geo64 = [&](int m, T cm) -> T {
            if (adj) {
                if (m <= min_lo) { const T t = (c_lo - cm) + d_lo; return t * t; }
                if (m >= max_hi) { const T t = (cm - c_hi) + d_hi; return t * t; }
                return geo_arg_adj<T>(m, lo, cm, c_lo, d_lo, c_hi, d_hi);
            }
            return geo_arg<T>(m, lo, hi, cm, c_lo, d_lo, c_hi, d_hi);
        };
        auto member = [&](const V4<T> &q, int m, auto ADJ, auto STORE) {
            if constexpr (sizeof(T) == 8) {
                // (fp64, round 6) Q is not accumulated pair by pair: with the wave's origin o, sum_m P_mn |x_n - y_m|^2 = Pt1_n |x_n - o|^2 + the nodes' part
                // sum_mk d_mk (s_mk + R_mk), d = o - y_m, formed in the column sums' fixed-point tail from the very sums it converts (k_estep2 has the algebra;
                // in fp64 the three parts' cancellation costs nothing that matters at the mode's 1e-7)
                T e = geo64(m, q.w) * k2;
                if (VIS) e += lvL[m];
                const T p = Num<T>::exp2(e);
                sum += p;
                if (decltype(STORE)::value) pb[(m - wlo) * kPStride + lane] = p;
            } else {
            T e = (decltype(ADJ)::value ? geo_arg_adj<T>(m, lo, q.w, c_lo, d_lo, c_hi, d_hi) : geo_arg<T>(m, lo, hi, q.w, c_lo, d_lo, c_hi, d_hi)) * k2;
            if (VIS) e += lvL[m];
            const T p = Num<T>::exp2(e);
            const T ddx = x - q.x, ddy = y - q.y, ddz = z - q.z;
            const T d2 = ddx * ddx + ddy * ddy + ddz * ddz;
            sum += p;
            qs += p * d2;
            if (decltype(STORE)::value) pb[(m - wlo) * kPStride + lane] = p;          // the chunks of the window that fit the tile
            }
        };
        // [from, to] in groups of 4 nodes: scalar loads first (clamped index), evaluations beyond `to` skipped wave-uniformly
        auto span = [&](int from, int to, auto ADJ, auto STORE) {
            if constexpr (LANE_NODES) {                  // (a node's four values from its lane: no scalar load in the loop)
                for (int m = from; m <= to; ++m) {
                    V4<T> q; q.x = lane_val(qn.x, m); q.y = lane_val(qn.y, m); q.z = lane_val(qn.z, m); q.w = lane_val(qn.w, m);
                    member(q, m, ADJ, STORE);
                }
                return;
            }
            int m0 = from;
            for (; m0 + 3 <= to; m0 += 4) {              // whole groups: one scalar load of four nodes (the scalar unit is shared by the
                const Node4<T> q4 = load_node4<T>(f.nodes, m0);          // CU's four SIMDs: index clamps, address arithmetic and a
#pragma unroll                                                           // wave-uniform branch per node had cost one scalar instruction
                for (int k = 0; k < 4; ++k) {                            // per two vector ones, SQ_INSTS_SALU 8.15 M : VALU 15.1 M)
                    V4<T> q; q.x = q4.v[4 * k]; q.y = q4.v[4 * k + 1]; q.z = q4.v[4 * k + 2]; q.w = q4.v[4 * k + 3];
                    member(q, m0 + k, ADJ, STORE);
                }
            }
            if (m0 <= to) {                              // the last, partial group: the same load, evaluations beyond `to` skipped
                const Node4<T> q4 = load_node4<T>(f.nodes, m0);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (m0 + k <= to) {
                        V4<T> q; q.x = q4.v[4 * k]; q.y = q4.v[4 * k + 1]; q.z = q4.v[4 * k + 2]; q.w = q4.v[4 * k + 3];
                        member(q, m0 + k, ADJ, STORE);
                    }
                }
            }
        };
        {
            const int wst = (wlo + RS - 1) < whi ? (wlo + RS - 1) : whi;              // last node whose membership is stored
            if (adj) { span(wlo, wst, std::true_type(), std::true_type()); span(wst + 1, whi, std::true_type(), std::false_type()); }
            else { span(wlo, wst, std::false_type(), std::true_type()); span(wst + 1, whi, std::false_type(), std::false_type()); }
        }
        ESTAMP(4);
        EPHASE(4);
        const T inv = valid ? Num<T>::rcp_fast(sum + cn) : T(0);
        // column sums are taken relative to a wave-local origin (lane 0's point; the sorted cloud keeps a
        // wave's points within centimetres) and leave as the residual R_m = sum_n P_mn (x_n - y_m):
        // small numbers, so fp32 tile sums lose nothing that matters (everything after a tile's sums is 64-bit fixed point)
        const T ox = bcast_first(x), oy = bcast_first(y), oz = bcast_first(z);
        if constexpr (sizeof(T) == 8) { const T ux = x - ox, uy = y - oy, uz = z - oz; qs = sum * (ux * ux + uy * uy + uz * uz); }      // Pt1_n |x_n - o|^2 (Pt1 = inv * sum)
        { const double qv = (double)(inv * qs); acc_ok &= __builtin_fabs(qv) < limQ; accQ += acc_fix(qv, scQ); }
        V4<T> pw; pw.x = inv; pw.y = inv * (x - ox); pw.z = inv * (y - oy); pw.w = inv * (z - oz);     // (s0, sx) and (sy, sz) pair up for v_pk_fma
        // one entry of padding after every 16 points: the column sums below read 16-point slices with all lanes of a slice on one
        // address (broadcast), and a ds_read_b128 serves 16 lanes that straddle two slices at a time -- 256 bytes apart they fall
        // on the same banks (2-way conflict on every read, SQ_LDS_BANK_CONFLICT = 69 % of the LDS cycles at N = 2 000 000),
        // 272 bytes apart they do not
        pts[wave * kPtsStride + lane + (lane >> 4)] = pw;

        {
            // ---- column sums (:386-389): lane = (node of the window, slice of the 64 points).  The window is summed in
            // chunks of kTileRows nodes (identical order in both tile variants, so a batch gives the bits of a single
            // frame): once sigma is millimetres the whole window is one chunk; the wide windows of the first iterations
            // take several.  With the small batch tile the memberships of the later chunks are recomputed (same
            // expression, same bits) instead of being kept in a 64-row tile.
            const int Wtot = whi - wlo + 1;
            for (int c0 = 0; c0 < Wtot; c0 += TR) {
            const int Wn = (Wtot - c0) < TR ? (Wtot - c0) : TR;
            const int wlo_c = wlo + c0;
            const bool rec = c0 >= RS;                                   // chunk beyond the stored part of the window
            const int rbase = rec ? 0 : c0;                              // first tile row of this chunk
            if (rec) {
#pragma unroll 4
                for (int m = wlo_c; m < wlo_c + Wn; ++m) {
                    const T cm = nodes[m].w;
                    T e;
                    if constexpr (sizeof(T) == 8) e = geo64(m, cm) * k2;
                    else e = (adj ? geo_arg_adj<T>(m, lo, cm, c_lo, d_lo, c_hi, d_hi) : geo_arg<T>(m, lo, hi, cm, c_lo, d_lo, c_hi, d_hi)) * k2;
                    if (VIS) e += lvL[m];
                    pb[(m - wlo_c) * kPStride + lane] = Num<T>::exp2(e);
                }
            }
            wave_lds_sync();
            // (a converged window is 5 to 8 nodes: with 8 lanes per slice a lane sums 8 points instead of 16, and the extra
            // level of the slice reduction is one DPP add per sum)
            const int shift = Wn <= 8 ? 3 : (Wn <= 16 ? 4 : 5);          // wave-uniform
            const int wl = lane & ((1 << shift) - 1), sl = lane >> shift;
            const int nj = 1 << shift;                                   // points per slice (= lanes per slice): 8 / 16 / 32
            T s0 = 0, sx = 0, sy = 0, sz = 0;
            if (wl < Wn) {
                for (int h = 0; h < nj; h += 8) {                        // 8 points at a time (same order as one loop over nj)
                    const int i0 = sl * nj + h;
                    const T *prow = pb + (rbase + wl) * kPStride + i0;
                    const V4<T> *pw_ = pts + wave * kPtsStride + i0 + (i0 >> 4);
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const T p = prow[j];
                        const V4<T> w = pw_[j];
                        s0 += p * w.x; sx += p * w.y; sy += p * w.z; sz += p * w.w;
                    }
                }
            }
            // ---- the slices' partial sums folded together, and the fixed-point tail with ONE value per lane.
            // s0 (the node's P1 share, which every residual needs) goes through plain butterfly steps: every lane of a node ends up with it.  The three
            // residual sums are FOLDED: fold32(sx, sy) puts sx's halves into lanes 0..31 and sy's into lanes 32..63 with one exchange, fold16 then
            // leaves row 0 with Sx, row 2 with Sy, rows 1 and 3 with Sz -- so that each row of 16 lanes converts a different value of its nodes:
            // row 0 Rx, row 1 Rz, row 2 Ry, row 3 P1 (from s0).  Same pairs added in the same order as the xor-32 / xor-16 / ror-8 butterflies of
            // before (same bits), in 12 cross-lane instructions instead of 8 trips through the LDS crossbar + 12 more; and the half-rate fp64
            // instructions of the tail (conversions, the residual's FMA, the range check, acc_fix) are issued once instead of four times.
            // (32-lane slices come in two: lanes 0..31 convert Rx then Rz, lanes 32..63 Ry then P1.)   R_k = s_k + (o_k - y_k) w0;  P1 = 0 + 1 w0.
            s0 = fold32(s0, s0);
            T u = fold32(sx, sy), v = fold32(sz, sz);
            if (shift <= 4) { s0 = fold16(s0, s0); u = fold16(u, v); }
            if (shift <= 3) { s0 += row_ror8(s0); u += row_ror8(u); }
            {
                typedef __attribute__((address_space(3))) long long lds_i64;
                const V4<T> ym = nodesL[wlo_c + (wl < Wn ? wl : 0)];
                lds_i64 *acn = (lds_i64 *)(accL + (size_t)(wlo_c + wl) * 4);
                const double w0 = (double)s0;
                const int grp = shift == 5 ? (lane >> 5) * 2 : (lane >> 4);          // which value(s) this lane converts: 0: Rx (then Rz), 1: Rz, 2: Ry (then P1), 3: P1
                const bool mine = wl < Wn && (shift != 3 || (lane & 8) == 0);         // (8-lane slices: both halves of a row hold the totals, the lower one converts)
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if (r == 1 && shift != 5) break;                 // (wave-uniform)
                    const int g = grp + r;                           // 0 Rx, 1 Rz, 2 Ry, 3 P1
                    const bool gx = g == 0, gy = g == 2, gp = g == 3;
                    const T sk = r == 0 ? u : v, ok = gx ? ox : (gy ? oy : oz), yk = gx ? ym.x : (gy ? ym.y : ym.z);
                    const int k = gx ? 1 : (gy ? 2 : (gp ? 0 : 3));
                    const double d = gp ? 1.0 : (double)ok - (double)yk, a = gp ? 0.0 : (double)sk;
                    const double val = ::fma(d, w0, a);
                    acc_ok &= !mine || __builtin_fabs(val) < (gp ? limP : limR);
                    // (ds_add_u64 without return: one LDS instruction per value instead of read, 64-bit add, write)
                    if (mine) __hip_atomic_fetch_add(acn + k, acc_fix(val, gp ? scP : scR), __ATOMIC_RELAXED, NCH == 1 ? __HIP_MEMORY_SCOPE_WAVEFRONT : __HIP_MEMORY_SCOPE_WORKGROUP);
                    if constexpr (sizeof(T) == 8) {      // the nodes' part of Q: d (s + R) per (node, coordinate); the P1 lanes add nothing of it
                        const double dq = (mine && !gp) ? d * (a + val) : 0.0;
                        acc_ok &= __builtin_fabs(dq) < limQn; accQ += acc_fix(dq, scQ);
                    }
                }
                wave_lds_sync();
            }
            }
        }
        EPHASE(5);
    }

    ESTAMP(5);
    // ---- the workgroup's share: its waves' integer sums added up, then into the accumulators of this iteration's parity, replica row =
    //      workgroup % kAccRows (integer atomics: neither the order of the waves nor that of the workgroups matters)
    long long *iscr = (long long *)scratch;
    {
        const long long qw = wave_sum_i64(accQ);
        if (lane == 0) iscr[wave] = qw;
    }
    if (__ballot(!acc_ok) != 0ull && lane == 0) {
        // a contribution beyond the fixed point's range, or not a number: the sums of this iteration are void.  The registration ends here with
        // an error (the M-step that follows finds done = 1 and leaves Y as it is) instead of continuing on wrapped-around integers.
        if constexpr (FUSED) f.sync[kFusedErrWord + hand->err_w] = f.host_epoch;      // (the state's copies belong to workgroup 0 of this launch: kFusedErrWord)
        else {
        IterState *sw = f.st;
        sw->status = TDLO_E_NUMERIC; sw->converged = 0; sw->done = 1;
        }
    }
    __syncthreads();
    ESTAMP(6);
    long long *arow = f.acc + ((size_t)(EARLY ? par_e : (TDLO_AS_GLOBAL(IterState, f.st)->it & 1)) * kAccRows + (blockIdx.x & ((FUSED ? hand->acc_rows : acc_rows_used(f)) - 1))) * acc_stride(M);
    {
        const long long *accAll = (const long long *)(scratch + 16);
        for (int i = tid; i < 4 * M; i += EB) {
            const int m = i >> 2, k = i & 3;
            long long v = 0;
            if (NCH == 1) {
#pragma unroll
                for (int w = 0; w < NWE; ++w) v += accAll[(size_t)w * M * 4 + i];
            } else {
                v = accAll[i];
            }
            acc_add(arow, k * M + m, v);
        }
    }
    if (tid == 0) {
        long long q = 0;
#pragma unroll
        for (int w = 0; w < NWE; ++w) q += iscr[w];
        acc_add(arow, 4 * M, q);
    }
    ESTAMP(7);
    EPHASE(7);
#ifdef TDLO_TIMELINE
    if (tid == 0 && tl_it >= 0 && tl_it < 8) atomicMax(&f.dbg[4 * tl_it + 1], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
#ifdef TDLO_ESTEP_PHASES
    if (tid == 0 && (int)blockIdx.x == f.nblkE / 2) { for (int i = 0; i < 10; ++i) f.dbg[48 + i] = ph_acc[i]; }
#endif
#ifdef TDLO_ESTEP_STAMPS
    if (tid == 0) atomicMax(&f.dbg[33], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
#undef ESTAMP
#undef EPHASE
