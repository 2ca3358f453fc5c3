// rocket_rmsprop_body.inc — the body of rr_a2c_update's RMSprop launch (a2c_rmsprop_kernel), kept as text
// beside rocket_ppo_adam_body.inc, whose one-tensor-per-wave addressing and clip_grad_norm_ coefficient it
// takes. In scope where it is included: the kernel's arguments (A, normw, n_norm, max_norm, lr_p, alpha,
// w, eps, eps_inside). After the clip (gradients scaled in place, as clip_grad_norm_ does), per element
//   sq = alpha sq + (1 - alpha) g g                      (w = 1 - alpha, from the host's double)
//   eps_inside 1  p -= lr g / sqrt(sq + eps)             SB3's RMSpropTFLike
//   eps_inside 0  p -= lr g / (sqrt(sq) + eps)           torch.optim.RMSprop
// on the optimizer's own square_avg tensors (A.exp_avg_sq; A.exp_avg is not read), and every tensor's step
// becomes the count the finish launch left after the sums (normw[n_norm]). No momentum, not centered, no
// weight decay; no next-minibatch blocks and no repacking (every rr_a2c_update packs for itself).
    __shared__ float red[kAdamThreads / kWave];
    // Every wave holds elements of one tensor (wstart: sizes rounded up to a wave), so the tensor and its
    // pointers are scalar. The element's three loads go first, unmasked (a padding lane reads element 0):
    // their round trip overlaps the norm's.
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int64_t wbase = (int64_t)blockIdx.x * kAdamThreads + (int64_t)wv * kWave;
    int t = 0;
    while (t + 1 < A.n && wbase >= A.wstart[t + 1]) ++t;
    const int64_t kw = wbase - A.wstart[t] + (threadIdx.x & (kWave - 1));
    const bool live = wbase < A.wstart[A.n] && kw < A.start[t + 1] - A.start[t];
    const int64_t k = live ? kw : 0;
    const float g0 = A.grad[t][k], s0 = A.exp_avg_sq[t][k], p0 = A.param[t][k];
    float part = 0.0f;
    for (int b = threadIdx.x; b < n_norm; b += kAdamThreads) part += normw[b];
    const float tot = block_sum<kAdamThreads>(part, red);
    const float step = normw[n_norm], lr = *lr_p;
    const float coef = max_norm > 0.0f ? fminf(max_norm / (sqrtf(tot) + 1e-6f), 1.0f) : 1.0f;
    if (live) {
        const float g = g0 * coef;
        A.grad[t][k] = g;
        const float sq = alpha * s0 + (w * g) * g;
        A.exp_avg_sq[t][k] = sq;
        const float den = eps_inside ? sqrtf(sq + eps) : sqrtf(sq) + eps;
        A.param[t][k] = p0 - lr * (g / den);
    }
    if (blockIdx.x == 0 && threadIdx.x < A.n) *A.step[threadIdx.x] = step;
