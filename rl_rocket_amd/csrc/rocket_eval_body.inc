// rocket_eval_body.inc — the body of the one-launch evaluation kernels, included as text inside the
// kernels that share it: eval_kernel (RR_EVAL_TRACE 0) and eval_trace_kernel (RR_EVAL_TRACE 1), both
// in rocket_eval.inc. Text and not a function: a body shared through a forceinlined __device__
// template, and one `if constexpr (TRACE)` body with the trace lambdas at function scope, each changed
// the machine code of one kernel family or the other (DESIGN.md, "Shared kernel bodies"); with #if
// regions each kernel sees exactly the token stream it had as a kernel of its own.
// In scope where it is included: the template parameters MODEL, INTEG, PREC, the kernel's arguments
// (state, n_envs, mode, P, B, io), RR_EVAL_TRACE defined to 0 or 1 and, with 1, the argument tr0
// (EvalTraceIO) and the trace declarations of rocket_eval.inc (TraceArgs, trace_args, trace_row,
// gfloat_t). The plain kernel never sees those names.
// RR_EVAL_TRACE 1 selects the five regions that record the envs with a trace slot: the slot's load,
// the recording lanes' setup with row 0 of episode 0, the step's record, row 0 of the next episode,
// and the length of an episode cut by max_steps.
// RR_DISCRETE_HEAD defined (rollout_discrete/rocket_rollout_discrete.hip: eval_discrete_kernel, which fixes
// MODEL 3 and PREC 0 and adds the arguments n_choices and tab, a DiscTable) selects the Categorical
// head: the pi tower's NH = 4 heads are logits and the action is the table row of the largest of the
// first n_choices. Not defined: the Gaussian head's clipped means.
// Both (eval_trace_discrete/rocket_eval_trace_discrete.hip: eval_discrete_trace_kernel, which adds the argument
// choice, an int32 plane [n_slots][n_episodes][steps] or nullptr) select one more region, seen by no other
// kernel: the head keeps the winner's index and the step's record stores it beside the action row, under
// the action row's t < steps rule. tr0 must stay the argument after io (trace_args reads it at that offset).
// RR_EVAL_SAMPLE defined (eval_sampled/rocket_eval_sampled.hip: eval_sampled_kernel and eval_sampled_trace_kernel;
// eval_sampled_discrete/rocket_eval_sampled_discrete.hip: their Categorical twins; no other kernel defines it)
// selects the regions that SAMPLE the action (SB3 evaluate_policy(deterministic=False)) where the others take
// the most likely one: the load of *iter at kernel entry, the noise key of the step, and in place of the
// clipped means the Gaussian sample, or inside RR_DISCRETE_HEAD in place of the argmax the softmax, the
// uniform draw and the inverse-CDF index with its table row (ci is then the sampled index). These lines are
// rocket_rollout_body.inc's sample regions, statement for statement, with t = the loop index k and without
// the log-prob, so an episode has the bits of the one rr_rollout_step / rr_rollout_step_discrete runs with
// the same (seed, *iter). They need three more arguments after every other one: seed_lo, seed_hi (uint32_t,
// the words of splitmix64(seed)) and iter (const uint64_t*).
    constexpr int NS = Dims<MODEL>::NS, NA = Dims<MODEL>::NA, NT = Dims<MODEL>::NT, EV = Dims<MODEL>::EV;
    constexpr int EPW = rol::Shape<2>::kEPW, NWV = rol::Shape<2>::kWaves;
#ifdef RR_DISCRETE_HEAD
    constexpr int NH = 4;   // heads of the packed image (rr_policy_pack_discrete): the logits
#else
    constexpr int NH = NA;  // heads: the action means
#endif
    using L = pol::Layout<NS, NH, PREC>;
    __shared__ __attribute__((aligned(16))) float sp[L::SIZE];
    __shared__ __attribute__((aligned(16))) float tile_all[NWV][EPW * NS];  // the post-call obs rows (and the trace's lane words)
    __shared__ __attribute__((aligned(16))) rol::ResetParams<NS> rps;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint32_t n = n_envs;
    const uint32_t wave_base = (blockIdx.x * NWV + wv) * EPW;
    // waves past n (last workgroup only) run on a clamped env, never evaluate and store nothing,
    // so every wave reaches the workgroup barrier below
    const bool live = wave_base < n;
    const uint32_t i = wave_base + lane;
    const bool valid = live && i < n;
    const uint32_t ic = i < n ? i : n - 1;
    const uint32_t vo = ic * 4u;
    const uint32_t plane = n * 4u;
    const uint32_t nvalid = !live ? 0u : ((n - wave_base) < (uint32_t)EPW ? (n - wave_base) : (uint32_t)EPW);
    const rsrc_t st_r = make_rsrc(state, (uint64_t)(NS + 3) * plane);
    const uint32_t v0_off = NS * plane, cw_off = (NS + 1) * plane, ret_off = (NS + 2) * plane;

    // ---- loads (as rollout_step_kernel; an auto-reset handle always keeps counter words) ----
    uint32_t cw = bld_u(st_r, vo, cw_off);
    float y0[NS], y1[NS], f0[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) y0[j] = bld_f(st_r, vo, j * plane);
    float v0 = bld_f(st_r, vo, v0_off);
    float ret = (mode & RR_FLAG_EPISODE_STATS) ? bld_f(st_r, vo, ret_off) : 0.0f;
#if RR_EVAL_TRACE
    const uint32_t slot0 = bld_u(make_rsrc(tr0.slot, plane), vo, 0);  // the env's trace slot
#endif
    pol::stage_params<NS, NH, PREC, rol::Shape<2>::kThreads>(io.params, sp);
    rol::stage_reset<NS>(B.kp, &rps);
    const HotParams H = load_hot<NS>(P);
    const CounterLayout CL(P);
    const int32_t n_ep = io.n_episodes;
#ifdef RR_EVAL_SAMPLE
    const uint64_t it = *iter;  // read once: the whole call draws under one iteration word
#endif
    int32_t ep = 0;            // episodes this env has completed
    float m0 = y0[NS - 1];     // mass at the first state of the running episode
    bool v0_new = false;
    float o[NS];
#if RR_EVAL_TRACE
    // ---- trace: a recording lane carries only its mask bit; the 64-bit row index is formed where
    // a row is stored, inside the branch only recording lanes take ----
    // a value outside [0, n_slots) records nothing (negative ones too: the compare is unsigned)
    const bool rec = valid && slot0 < (uint32_t)tr0.n_slots;
    // Each lane's slot and step count live in LDS, not in registers: the 6DOF loop sits at the
    // 256-VGPR line of two waves per SIMD (eval_kernel<6, RK4, fp32>: 254), and two more values
    // live across the policy's MFMAs cost the second wave or spilled to scratch. They use the
    // wave's obs tile, which is idle until the loop has ended (words [0, 64) and [64, 128) of
    // >= 448), so the workgroup's LDS stays eval_kernel's. Only recording lanes touch these words,
    // in the branch that stores a row. volatile: a load hoisted out of the loop would put the
    // value back into a register.
    // lane_t: steps of the running episode taken in THIS call (the counter word's field may start above 0)
    static_assert(EPW * NS >= 2 * kWave, "the wave's obs tile holds lane_slot and lane_t");
    typedef volatile __attribute__((address_space(3))) uint32_t lds_word_t;
    lds_word_t* const lane_slot = (lds_word_t*)tile_all[wv];
    lds_word_t* const lane_t = lane_slot + kWave;
    lane_slot[lane] = slot0;
    lane_t[lane] = 0;
    // episodes ahead of (slot, ep) in the buffers; times rows per episode this may pass 2^32
    // this lane's word of lane_slot / lane_t, formed where it is used from values the loop keeps
    // anyway (the opaque asm keeps the LDS address from being hoisted into a register of its own)
    auto lane_word = [&]() {
        uint32_t w = lane;
        asm volatile("" : "+v"(w));
        return w;
    };
    auto episode_index = [&](uint32_t slot) { return (uint64_t)slot * (uint32_t)n_ep + (uint32_t)ep; };
    if (rec) trace_row<NS>(tr0.state + episode_index(slot0) * ((uint32_t)tr0.steps + 1u) * NS, y0);  // row 0 of episode 0
#endif
    __syncthreads();  // packed policy and reset parameters staged

    for (uint64_t k = 0; k < io.max_steps; ++k) {
        const bool active = valid && ep < n_ep;
        if (__ballot(active) == 0) break;

#ifdef RR_EVAL_SAMPLE
        // ---- sampled action: the pi tower's means or logits, then rollout_step_kernel's sample of step t = k ----
#else
        // ---- deterministic action: the pi tower's means, clipped ----
#endif
        normalize_obs<NS>(y0, H.inv_norm, o);
        float value, mean[NH], a_env[NA];
        typename pol::XOp<PREC>::T x[2][L::KP1];
        rol::regs_x<NS, NH, PREC>(o, x);
        rol::policy_forward<NS, NH, PREC, 2, false>(sp, x, lane, value, mean);
#ifdef RR_EVAL_SAMPLE
        // sample: the key and arithmetic of policy_act_kernel (rocket_rollout_body.inc's lines)
        const uint32_t t = (uint32_t)k;
        uint32_t key = mix32((uint32_t)(P.id_off + i) ^ seed_lo);
        key = mix32(key ^ (uint32_t)it ^ seed_hi);
        key = mix32(key ^ (uint32_t)(it >> 32) ^ (t * 0x9E3779B9u));
#endif
#if defined(RR_DISCRETE_HEAD) && defined(RR_EVAL_SAMPLE)
        // The Categorical head's sample: discrete_act_kernel's lines as rocket_rollout_body.inc has them, without
        // the log-prob. Softmax over the first n_choices logits
        float zm = mean[0];
#pragma unroll
        for (int q = 1; q < NH; ++q) zm = q < n_choices ? fmaxf(zm, mean[q]) : zm;
        float ex[NH], sum = 0.0f;
#pragma unroll
        for (int q = 0; q < NH; ++q) {
            ex[q] = q < n_choices ? expf(mean[q] - zm) : 0.0f;
            sum += ex[q];
        }
        const float u = (float)(mix32(key) >> 8) * 0x1p-24f;  // one uniform per env, [0, 1)
        // index = the number of q in 0 .. K - 2 whose running sum p_0 + .. + p_q is <= u and which have a
        // positive weight beyond them: a choice whose weight underflowed to 0 is never drawn
        const int index = categorical_index(ex, sum, u, n_choices);
        // the table row by compares: no data-dependent address
        a_env[0] = tab.v[0][0];
        a_env[1] = tab.v[0][1];
#pragma unroll
        for (int q = 1; q < NH; ++q)
            if (index == q) {
                a_env[0] = tab.v[q][0];
                a_env[1] = tab.v[q][1];
            }
#if RR_EVAL_TRACE
        const int32_t ci = index;  // the sampled index, for the trace's choice plane
#endif
#elif defined(RR_DISCRETE_HEAD)
        // the most probable choice: the lowest q < n_choices with the largest logit (torch.argmax: on a tie
        // the lowest index; a zero-packed head >= n_choices never wins), then its table row by compares
        float zb = mean[0];
        a_env[0] = tab.v[0][0];
        a_env[1] = tab.v[0][1];
#if RR_EVAL_TRACE
        int32_t ci = 0;  // the winner's index, for the trace's choice plane
#endif
#pragma unroll
        for (int q = 1; q < NH; ++q)
            if (q < n_choices && mean[q] > zb) {
                zb = mean[q];
                a_env[0] = tab.v[q][0];
                a_env[1] = tab.v[q][1];
#if RR_EVAL_TRACE
                ci = q;
#endif
            }
#elif defined(RR_EVAL_SAMPLE)
        float eps[NA];
#pragma unroll
        for (int a = 0; a < NA; a += 2) {
            const float2 z = pol::normal2(key + (uint32_t)a * 0x632BE5ABu);
            eps[a] = z.x;
            if (a + 1 < NA) eps[a + 1] = z.y;
        }
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const float ls = sp[L::LS + a];
            const float act = mean[a] + __builtin_amdgcn_exp2f(ls * 1.44269504088896341f) * eps[a];
            a_env[a] = fminf(1.0f, fmaxf(-1.0f, act));  // the env steps with the clipped sample
        }
#else
#pragma unroll
        for (int a = 0; a < NA; ++a) a_env[a] = fminf(1.0f, fmaxf(-1.0f, mean[a]));
#endif

        if (active) {
            // ---- env step (rollout_step_kernel / step_kernel) ----
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

#if RR_EVAL_TRACE
            // ---- trace: the step's record (row t + 1 of the states: the un-reset y1) ----
            if (rec) {
                const TraceArgs tr = trace_args();
                const uint32_t cap = tr.steps;
                const uint32_t lw = lane_word();
                const uint32_t slot = lane_slot[lw], t = lane_t[lw];
                if (t < cap) {  // steps past the capacity are counted, not written
                    const uint64_t e = episode_index(slot);
                    trace_row<NS>(tr.state + (e * (cap + 1u) + t + 1u) * NS, y1);
                    const uint64_t row = e * cap + t;
                    if (tr.action) trace_row<NA>(tr.action + row * NA, a_env);
#ifdef RR_DISCRETE_HEAD
                    if (choice) choice[row] = ci;  // the index whose table row that is
#endif
                    if (tr.terms) {
                        gfloat_t* tp = tr.terms + row * (NT + 1);
                        trace_row<NT>(tp, tt);
                        trace_row<1>(tp + NT, &r);
                    }
                }
                lane_t[lw] = done ? 0u : t + 1u;
                if (done) tr.length[(uint64_t)ep * tr.n_slots + slot] = (int32_t)(t + 1u);
            }

#endif
            if (done) {
                // ---- the episode's row, then the auto-reset of the step kernels ----
                const size_t row = (size_t)ep * n + i;
                if (io.ep_return) io.ep_return[row] = ret;
                if (io.ep_length) io.ep_length[row] = el;
                if (io.flags)
                    io.flags[row] = (uint8_t)((event ? RR_EVAL_EVENT : 0) | (bv ? RR_EVAL_BOUNDS : 0) |
                                              (trunc ? RR_EVAL_TRUNCATED : 0) | (nf ? RR_EVAL_NONFINITE : 0) |
                                              (tt[NT - 1] != 0.0f ? RR_EVAL_LANDED : 0));
                if (io.used_mass) io.used_mass[row] = m0 - y1[NS - 1];
                if (io.final_state) {
                    float* fs = io.final_state + (size_t)ep * NS * n + i;
#pragma unroll
                    for (int j = 0; j < NS; ++j) fs[(size_t)j * n] = y1[j];
                }
                ResetStream key = reset_stream(rps.seed_w, P.id_off + i, cw);  // cw is still this step's word
                sample_ic<MODEL>(rps, key, y1, v0);
                v0_new = true;
                cw = CL.next_episode(cw);
                el = 0;
                ret = 0.0f;
                m0 = y1[NS - 1];
                ++ep;
#if RR_EVAL_TRACE
                // ---- trace: row 0 of the next episode is the auto-reset state ----
                if (rec && ep < n_ep) {
                    const TraceArgs tr = trace_args();
                    trace_row<NS>(tr.state + episode_index(lane_slot[lane_word()]) * (tr.steps + 1u) * NS, y1);
                }
#endif
            }
            cw = CL.with_elapsed(cw, el);
#pragma unroll
            for (int j = 0; j < NS; ++j) y0[j] = y1[j];
        }
    }

    // ---- env state, counter word, running return; episodes completed ----
    if (valid) {
#pragma unroll
        for (int j = 0; j < NS; ++j) bst_f(st_r, y0[j], vo, j * plane);
        if (v0_new) bst_f(st_r, v0, vo, v0_off);
        bst_u(st_r, cw, vo, cw_off);
        if (mode & RR_FLAG_EPISODE_STATS) bst_f(st_r, ret, vo, ret_off);
        io.episodes[i] = ep;
    }
#if RR_EVAL_TRACE
    // ---- trace: an episode cut by max_steps reports the steps it took so far ----
    if (rec && ep < n_ep) {
        const TraceArgs tr = trace_args();
        const uint32_t lw = lane_word();
        tr.length[(uint64_t)ep * tr.n_slots + lane_slot[lw]] = (int32_t)lane_t[lw];
    }
#endif
    if (io.obs) {  // the post-call obs (of the fresh episode's first state where the env finished)
        normalize_obs<NS>(y0, H.inv_norm, o);
        store_obs_tile<NS, EPW>(tile_all[wv], o, make_rsrc(io.obs, (uint64_t)NS * plane), wave_base, lane, nvalid,
                                io.obs_vec_ok);
    }
