// rocket_rollout_body.inc — the body of the rollout kernels, included as text inside the kernels that
// share it: rollout_step_kernel (rocket_rollout.inc; RR_COLLECT_STATS 0) and
// rollout_collect_stats_kernel (collect_stats/rocket_collect_stats.inc; RR_COLLECT_STATS 1). Text and
// not a function: a body shared through a forceinlined __device__ template changed the machine code
// of the kernels that existed before it (DESIGN.md, "Shared kernel bodies"); with #if regions each
// kernel sees exactly the token stream it had as a kernel of its own.
// In scope where it is included: the template parameters or constants MODEL, INTEG, PREC, MULTI, NTW,
// the kernel's arguments (state, n_envs, mode, P, B, io), RR_COLLECT_STATS defined to 0 or 1 and,
// with 1, namespace rst and the argument sio (CollectStatsIO); MULTI must then be true and NTW 2.
// RR_COLLECT_STATS 1 selects the lines that account for the episodes the launch finishes: the lanes'
// LDS columns acc (declared last, so sp, tile_all and rps lie where the plain kernel has them), their
// initialisation, the accounting of a finished episode inside the done branch, and at the end of the
// rollout the sample sums ss of the GAE scan (always run: the call requires buf_adv), the wave's
// butterfly fold and its row of partials.
// The RR_ST / RR_ACC_* stamp hooks (rocket_stamps.h) expand to nothing in the shipped library; in a
// diagnostic build (RR_DIAG_STAMPS) the statistics kernel carries them too and, like the collect,
// then overwrites io.last_value of each wave's first 16 envs.
// RR_DISCRETE_HEAD defined (rollout_discrete/rocket_rollout_discrete.hip: rollout_discrete_kernel, which fixes
// MODEL 3, PREC 0, NTW 2 and adds the arguments n_choices and tab, a DiscTable) selects the Categorical
// head of the reference's DiscreteActions3DOF: the pi tower's NH = 4 heads are logits, of which the
// first n_choices count, the sample region is discrete_act_kernel's (one uniform draw, the index, the
// table row) and buf_act holds one float per sample, the index. Not defined: the Gaussian head.
// Both at once (collect_stats_discrete/rocket_collect_stats_discrete.hip: rollout_discrete_stats_kernel, with
// rollout_discrete_kernel's arguments and sio) need no region of their own: the two sets share no line.
    constexpr int NS = Dims<MODEL>::NS, NA = Dims<MODEL>::NA, NT = Dims<MODEL>::NT, EV = Dims<MODEL>::EV;
    constexpr int EPW = rol::Shape<NTW>::kEPW, NWV = rol::Shape<NTW>::kWaves;
#ifdef RR_DISCRETE_HEAD
    constexpr int NH = 4;   // heads of the packed image (rr_policy_pack_discrete): the logits
#else
    constexpr int NH = NA;  // heads: the action means
#endif
    using L = pol::Layout<NS, NH, PREC>;
    __shared__ __attribute__((aligned(16))) float sp[L::SIZE];
    __shared__ __attribute__((aligned(16))) float tile_all[NWV][EPW * NS];
    __shared__ __attribute__((aligned(16))) rol::ResetParams<NS> rps;
#if RR_COLLECT_STATS
    __shared__ __attribute__((aligned(16))) uint64_t acc[rst::Q_N][rol::Shape<NTW>::kThreads];  // the lanes' episode sums
#endif
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t n = n_envs;
    const uint32_t wave_idx = blockIdx.x * NWV + wv;
    const uint32_t wave_base = wave_idx * EPW;
    float* tile = tile_all[wv];
    // waves past n (last workgroup only) run on a clamped env and store nothing, so every
    // wave reaches the workgroup barrier below
    const bool live = wave_base < n;
    const uint32_t i = wave_base + (lane & (EPW - 1));  // NTW 1: lane l + 32 mirrors lane l
    const bool valid = live && i < n && lane < (uint32_t)EPW;
    const uint32_t ic = i < n ? i : n - 1;
    const uint32_t vo = ic * 4u;
    const uint32_t plane = n * 4u;
    const uint32_t nvalid = !live ? 0u : ((n - wave_base) < (uint32_t)EPW ? (n - wave_base) : (uint32_t)EPW);
    const bool use_counter = mode & kModeCounter;
    const rsrc_t st_r = make_rsrc(state, (uint64_t)(NS + 3) * plane);
    const uint32_t v0_off = NS * plane, cw_off = (NS + 1) * plane, ret_off = (NS + 2) * plane;
    // MULTI (rr_rollout_collect): io.T steps in this launch; the env state, counter word,
    // episode return and done flag stay in registers between steps and the rollout buffers
    // are [T][n] slices. Step k computes exactly what launch k of rr_rollout_step computes.
    const uint32_t T = MULTI ? io.T : 1u;

#if RR_COLLECT_STATS
    // this lane's column starts empty (only this lane reads or writes it before the end)
    const uint32_t tx = threadIdx.x;
#pragma unroll
    for (int w = 0; w < rst::Q_N; ++w) acc[w][tx] = 0ull;
    acc[rst::Q_MIN_MAX][tx] = rst::pair_f(INFINITY, -INFINITY);

#endif
    RR_ACC_BEGIN(16);
    // ---- loads (as step_kernel) ----
    uint32_t cw = use_counter ? bld_u(st_r, vo, cw_off) : 0u;
    float y0[NS], y1[NS], f0[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y0[j] = bld_f(st_r, vo, j * plane);
    float v0 = bld_f(st_r, vo, v0_off);
    float ret = (mode & RR_FLAG_EPISODE_STATS) ? bld_f(st_r, vo, ret_off) : 0.0f;
    bool start = io.done[ic] != 0;
    pol::stage_params<NS, NH, PREC, rol::Shape<NTW>::kThreads>(io.params, sp);
    if (mode & RR_FLAG_AUTO_RESET) rol::stage_reset<NS>(B.kp, &rps);
    const HotParams H = load_hot<NS>(P);
    const CounterLayout CL(P);
    const uint64_t it = *io.iter;
    float o[NS];
    bool v0_new = false;
    RR_ST(15);

    for (uint32_t k = 0; k < T; ++k) {
        const bool last = k + 1 == T;
        const size_t so = MULTI ? (size_t)k * n : 0;  // [T][n] slice of step k

        // ---- obs of step t: rollout buffer + MFMA operands ----
        normalize_obs<NS>(y0, H.inv_norm, o);
        if (MULTI && k > 0) {  // the tile's readers of the previous step are done
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        const rsrc_t bobs_r = make_rsrc(io.buf_obs + so * NS, (uint64_t)NS * plane);
        rol::ObsRead<NS, EPW> obr;
        if constexpr (kPolPrefetchA) rol::obs_begin<NS, EPW>(tile, o, bobs_r, wave_base, lane, nvalid, io.buf_obs_vec_ok, obr);
        else store_obs_tile<NS, EPW>(tile, o, bobs_r, wave_base, lane, nvalid, io.buf_obs_vec_ok);  // main TU: registers
        if (k == 0) __syncthreads();  // packed policy and reset parameters staged (T is uniform)

        // ---- policy (rocket_policy.inc towers on two 32-env tiles; env = lane) ----
        const int half = lane >> 5;
        float value, mean[NH];
        typename pol::XOp<PREC>::T x[NTW][L::KP1];
        if constexpr (NTW == 2) rol::regs_x<NS, NH, PREC>(o, x);
        else pol::load_x<NS, NH, PREC, NTW>(tile, lane, x);
        RR_ST(0);
        // collect TU: the obs rows' buffer stores are issued after the value tower's layer-1 MFMAs
        rol::policy_forward<NS, NH, PREC, NTW>(sp, x, lane, value, mean, [&](int p) {
            if constexpr (kPolPrefetchA)
                if (p == 1) rol::obs_end<NS, EPW>(obr, bobs_r, wave_base, lane);
            RR_ST(p);
        });
        // sample: the key and arithmetic of policy_act_kernel
        const uint32_t t = io.t + k;
        uint32_t key = mix32((uint32_t)(P.id_off + i) ^ io.seed_lo);
        key = mix32(key ^ (uint32_t)it ^ io.seed_hi);
        key = mix32(key ^ (uint32_t)(it >> 32) ^ (t * 0x9E3779B9u));
#ifdef RR_DISCRETE_HEAD
        // The Categorical head: discrete_act_kernel's lines (discrete/rocket_discrete.hip, the twin), statement
        // for statement, so that the index, the log-prob and the table row have its bits. Softmax over the
        // first n_choices logits; log p_k from the log of the sum (a p_k that underflows to 0 leaves log p_k
        // finite)
        float zm = mean[0];
#pragma unroll
        for (int q = 1; q < NH; ++q) zm = q < n_choices ? fmaxf(zm, mean[q]) : zm;
        float ex[NH], sum = 0.0f;
#pragma unroll
        for (int q = 0; q < NH; ++q) {
            ex[q] = q < n_choices ? expf(mean[q] - zm) : 0.0f;
            sum += ex[q];
        }
        const float lse = logf(sum);
        const float u = (float)(mix32(key) >> 8) * 0x1p-24f;  // one uniform per env, [0, 1)
        // index = the number of q in 0 .. K - 2 whose running sum p_0 + .. + p_q is <= u and which have a
        // positive weight beyond them: a choice whose weight underflowed to 0 is never drawn
        const int index = categorical_index(ex, sum, u, n_choices);
        // the chosen logit and the table row by compares: no data-dependent address
        float za = mean[0], a_env[NA] = {tab.v[0][0], tab.v[0][1]};
#pragma unroll
        for (int q = 1; q < NH; ++q)
            if (index == q) {
                za = mean[q];
                a_env[0] = tab.v[q][0];
                a_env[1] = tab.v[q][1];
            }
        const float act[1] = {(float)index}, lp = (za - zm) - lse;
#else
        float eps[NA];
#pragma unroll
        for (int a = 0; a < NA; a += 2) {
            const float2 z = pol::normal2(key + (uint32_t)a * 0x632BE5ABu);
            eps[a] = z.x;
            if (a + 1 < NA) eps[a + 1] = z.y;
        }
        float act[NA], a_env[NA], lp = 0.0f;
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const float ls = sp[L::LS + a];
            act[a] = mean[a] + __builtin_amdgcn_exp2f(ls * 1.44269504088896341f) * eps[a];
            lp += -0.5f * eps[a] * eps[a] - ls - 0.918938533204672742f;
            a_env[a] = fminf(1.0f, fmaxf(-1.0f, act[a]));
        }
#endif

        RR_ST(9);
        // ---- env step (step_kernel) ----
        const Ctl c = make_ctl<MODEL>(P, a_env);
        integrate<MODEL, INTEG>(P, c, y0, P.h, y1, f0);
        const float g0 = y0[EV], g1 = y1[EV];
        const bool event = (g0 <= 0.0f && g1 >= 0.0f) || (g0 >= 0.0f && g1 <= 0.0f);
        if (event) event_step<MODEL, INTEG>(P, c, y0, f0, y1);
        post_integrate<MODEL>(y1);
        bool bv;
        float tt[NT];
        const float r = reward_terms<MODEL>(H, y1, a_env, v0, bv, tt);
        const bool nf = nonfinite<NS>(y1);
        bool done = event || bv || nf, trunc;
        int32_t el = CL.time_limit(cw, done, trunc);
        ret += r;
        normalize_obs<NS>(y1, H.inv_norm, o);  // terminal obs where done
        RR_ST(10);

        // ---- timeout bootstrap from the terminal obs (waves holding a truncated env only) ----
        float rb = r;
        if (__ballot(trunc && valid)) {
            rol::put_rows<NS, NTW>(tile, o, lane);
            const float vt = rol::tile_value<NS, NH, PREC, NTW>(sp, tile, lane);
            rb = trunc ? fmaf(io.gamma, vt, r) : r;
        }

        RR_ST(11);
        // ---- done compaction, terminal rows, auto-reset (step_kernel) ----
        const bool dv = done && valid;
        const uint64_t m = __ballot(dv);
        if (last && lane == 0 && live) {
            if constexpr (NTW == 2) B.done_bits[wave_idx] = m;
            else reinterpret_cast<uint32_t*>(B.done_bits)[wave_idx] = (uint32_t)m;  // half of a 64-env word
        }
        if (m) {
            if (dv) {
                float* tr = B.term_obs + (size_t)i * NS;
#pragma unroll
                for (int j = 0; j < NS; ++j) tr[j] = o[j];
                B.term_ret[i] = ret;
                B.term_len[i] = el;
#if RR_COLLECT_STATS
                // the finished episode into this lane's column (before the auto-reset clears ret / el)
                acc[rst::Q_EP_LEN][tx] += rst::pair(1u, (uint32_t)el);
                acc[rst::Q_LANDED_EVENT][tx] += rst::pair(tt[NT - 1] != 0.0f, event);
                acc[rst::Q_BOUNDS_TRUNC][tx] += rst::pair(bv, trunc);
                acc[rst::Q_NONFIN][tx] += nf ? 1ull : 0ull;
                const uint64_t mm = acc[rst::Q_MIN_MAX][tx];
                acc[rst::Q_MIN_MAX][tx] = rst::pair_f(fminf(rst::lo_f(mm), ret), fmaxf(rst::hi_f(mm), ret));
                const double rd = (double)ret;
                acc[rst::Q_SUM][tx] = __builtin_bit_cast(uint64_t, __builtin_bit_cast(double, acc[rst::Q_SUM][tx]) + rd);
                acc[rst::Q_SQ][tx] = __builtin_bit_cast(uint64_t, __builtin_bit_cast(double, acc[rst::Q_SQ][tx]) + rd * rd);
#endif
            }
            if ((mode & RR_FLAG_AUTO_RESET) && dv) {
                // the auto-reset candidate, drawn by the done lanes only (key: cw is still this
                // step's word, as in step_kernel); waves without a done lane skip its ~190 VALU
                ResetStream key = reset_stream(rps.seed_w, P.id_off + i, cw);
                sample_ic<MODEL>(rps, key, y1, v0);
                if constexpr (MULTI) v0_new = true;
                else bst_f(st_r, v0, vo, v0_off);
                cw = CL.next_episode(cw);
                normalize_obs<NS>(y1, H.inv_norm, o);
                el = 0;
                ret = 0.0f;
            }
        }
        cw = CL.with_elapsed(cw, el);
        RR_ST(12);

        // ---- rollout buffer slices of step k; env outputs of the last step ----
        if (valid) {
#ifdef RR_DISCRETE_HEAD
            io.buf_act[so + i] = act[0];  // [T][n]: the index as a float (SB3's buffer of a Discrete space)
#else
#pragma unroll
            for (int a = 0; a < NA; ++a) io.buf_act[(so + i) * NA + a] = act[a];
#endif
            io.buf_val[so + i] = value;
            io.buf_logp[so + i] = lp;
            io.buf_start[so + i] = start ? 1.0f : 0.0f;
            io.buf_rew[so + i] = rb;
            if (last) {
                io.reward[i] = r;
                io.done[i] = (uint8_t)done;
                if (io.truncated) io.truncated[i] = (uint8_t)trunc;
                if (io.terms) {
#pragma unroll
                    for (int j = 0; j < NT; ++j) io.terms[(size_t)j * n + i] = tt[j];
                    io.terms[(size_t)NT * n + i] = bv ? 1.0f : 0.0f;
                    io.terms[(size_t)(NT + 1) * n + i] = event ? 1.0f : (nf ? -1.0f : 0.0f);  // solve_ivp status
                }
            }
        }
        start = done;
#pragma unroll
        for (int j = 0; j < NS; ++j) y0[j] = y1[j];
        RR_ST(13);
    }

    // ---- env state (the post-step, post-reset state of the last step) ----
    if (valid) {
#pragma unroll
        for (int j = 0; j < NS; ++j) bst_f(st_r, y0[j], vo, j * plane);
        if (v0_new) bst_f(st_r, v0, vo, v0_off);
        if (use_counter) bst_u(st_r, cw, vo, cw_off);
        if (mode & RR_FLAG_EPISODE_STATS) bst_f(st_r, ret, vo, ret_off);
    }
    if (io.obs) {  // post-step (post-reset) obs, e.g. on the last step of a rollout
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        store_obs_tile<NS, EPW>(tile, o, make_rsrc(io.obs, (uint64_t)NS * plane), wave_base, lane, nvalid,
                                  io.obs_vec_ok);
    }
    if constexpr (MULTI) {
        // ---- end of the rollout: V(last obs) (rr_policy_bootstrap), the SB3 episode-start /
        // last-done flags and GAE (rr_gae) of this env ----
        rol::put_rows<NS, NTW>(tile, o, lane);
        const float lv = rol::tile_value<NS, NH, PREC, NTW>(sp, tile, lane);
#if RR_COLLECT_STATS
        double ss[4] = {0.0, 0.0, 0.0, 0.0};  // sum y, y^2, d, d^2 of this env's samples
#endif
        if (valid) {
            const float ld = start ? 1.0f : 0.0f;
            if (io.last_value) io.last_value[i] = lv;
            if (io.last_done) io.last_done[i] = ld;
            if (io.last_start) io.last_start[i] = ld;
#if RR_COLLECT_STATS
            pol::gae_env_scan<true>(T, n, i, io.buf_rew, io.buf_val, io.buf_start, lv, ld, io.gamma64, io.lam,
                                    io.buf_adv, io.buf_ret, ss);
#else
            if (io.buf_adv)
                pol::gae_env(T, n, i, io.buf_rew, io.buf_val, io.buf_start, lv, ld, io.gamma64, io.lam, io.buf_adv,
                             io.buf_ret);
#endif
        }
        RR_ST(14);
        RR_ACC_WRITE(io.last_value, wave_base, lane, live && wave_base + lane < n && io.last_value);
#if RR_COLLECT_STATS

        // ---- the wave's row. Every lane takes its column out of LDS (its own words: no barrier),
        // the wave folds the 15 accumulated slots by butterfly, lane s < 16 stores slot s ----
        if (live) {
            uint64_t v[rst::kSlots - 1];
            const uint64_t q0 = acc[rst::Q_EP_LEN][tx], q1 = acc[rst::Q_LANDED_EVENT][tx], q2 = acc[rst::Q_BOUNDS_TRUNC][tx];
            const uint64_t q4 = acc[rst::Q_MIN_MAX][tx];
            v[RR_RSTAT_EPISODES] = (uint32_t)q0;
            v[RR_RSTAT_LEN_SUM] = q0 >> 32;
            v[RR_RSTAT_LANDED] = (uint32_t)q1;
            v[RR_RSTAT_END_EVENT] = q1 >> 32;
            v[RR_RSTAT_END_BOUNDS] = (uint32_t)q2;
            v[RR_RSTAT_END_TRUNCATED] = q2 >> 32;
            v[RR_RSTAT_END_NONFINITE] = acc[rst::Q_NONFIN][tx];
            v[RR_RSTAT_RET_SUM] = acc[rst::Q_SUM][tx];
            v[RR_RSTAT_RET_SQ] = acc[rst::Q_SQ][tx];
            v[RR_RSTAT_RET_MIN] = __builtin_bit_cast(uint64_t, (double)rst::lo_f(q4));
            v[RR_RSTAT_RET_MAX] = __builtin_bit_cast(uint64_t, (double)rst::hi_f(q4));
#pragma unroll
            for (int q = 0; q < 4; ++q) v[RR_RSTAT_Y_SUM + q] = __builtin_bit_cast(uint64_t, ss[q]);
            rst::wave_fold(v);
            uint64_t mine = (uint64_t)T * nvalid;  // RR_RSTAT_SAMPLES
#pragma unroll
            for (int q = 0; q < rst::kSlots - 1; ++q) mine = lane == (uint32_t)q ? v[q] : mine;
            if (lane < (uint32_t)rst::kSlots) sio.partials[(size_t)wave_idx * rst::kSlots + lane] = mine;
        }
#endif
    }
