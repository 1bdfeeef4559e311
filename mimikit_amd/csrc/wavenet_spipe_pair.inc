// The stage pipeline with TWO CLIPS PER VISIT (included by wavenet_spipe.hip, inside its namespace: same stages, placement, register images,
// messages, rings and head as the one-clip form above).
//
// Why.  From ~40 clips on the one-clip ring goes at a stage's beat, and the beat is made inside a CU: ~1.0 us per clip whether a stage waits
// for its messages or not (timing builds, 128 clips: free-running 1.01 us per visit; helper waves alone 0.97; chain waves alone 0.88; the
// helpers' bare loop - looks, staging, hand-shakes, no products - 0.60).  A visit's arithmetic is a third of that (88 packed FMAs and 32
// 4x4x1 matrix instructions per SIMD); the rest is what a visit costs whatever it carries: the looks' round trips, the LDS hand-shakes between
// the two waves of a SIMD, the reduce-scatter's DPP chain, exp2 / rcp, the stores.  So a visit carries two clips here:
//   * the LDS image of a visit holds the two clips' values of a channel side by side; a weight register pair is multiplied with them by
//     v_pk_fma_f32 with the weight broadcast by op_sel - the two halves of a packed accumulator are the two CLIPS (in the one-clip form they
//     are two halves of K), so a lane's accumulators and weights are the same registers as before, with twice the FMAs behind every LDS read;
//   * the reduce-scatter over the 16 lanes of a DPP row ends with a scatter over the clip instead of an all-reduce: of the four lanes that
//     held a gate row's total, two now hold clip 0's and two clip 1's - gate, publish, ring store and hand-over are the same instructions
//     with twice the lanes active;
//   * the helpers look for, stage and hand over two messages per duty, ask for two clips' rows per request, and a batch of four biases on
//     the matrix pipe (v_mfma_f32_4x4x1) is two visits.
// Arithmetic: a gate row's 512 products are added up in ONE chain per lane slice (the one-clip form: two, added at the end) - results differ
// from the one-clip form by rounding, like the 16-clip groups' do.
// Reference: wavenet_v2.py:131-182, :276-293 (see the head of wavenet_spipe.hip).

constexpr int kSlice2 = 36;                    // a K slice of 16 channels x 2 clips (32 floats) + 4 of padding: the 16 slices' 16-byte reads fall on different banks
constexpr int kHalf2 = 16 * kSlice2;           // 576 floats: C channels of two clips, {clip 0, clip 1} per channel
__device__ __forceinline__ int pad2_of(int ch) { return (ch >> 4) * kSlice2 + (ch & 15) * 2; }

constexpr int kRowsbDepth = 2;                 // a power of two (4 deep: 128 clips 103.2 -> 105.2 us per step)
struct Lds2 {
  float xy[kXyRing][2 * kHalf2];              // the newest visits' messages: [x | y], two clips interleaved
  float rowsb[kRowsbDepth][4][kBRow];         // the rows of a BATCH of four clip-visits (= two visits): [x_s[t - d] (256) | c[t] (256)] + padding; a batch's rows are staged
                                              // once every helper is through with the batch kRowsbDepth before it (two: the four helpers go in lock step, one iteration of slack)
  unsigned arrived[4];                        // [v mod 4]: v + 1 once the two messages of visit v are staged
  unsigned hdone[4];                          // per chain wave: visits whose image it no longer needs
  unsigned ready[4];                          // per helper: biases prepared, in CLIP-visits (step * B + clip)
  unsigned hidin_ready[4];                    // [v mod 4]: v + 1 once the hidden units' hand-over of the stage below is staged for visit v
  unsigned rows_ready[8];                     // [clip-visit mod 8]: clip-visit + 1 once its rows are staged (eight words: each has ONE writer, so it only grows)
  float hidin[kXyRing][2][16];                // the hand-over: this CU's 16 units, per clip
  float bias[];                               // as in the one-clip form: [chain wave][step parity][Bcap clips][gate row]
};

// acc{clip 0, clip 1} += w.lo * x{clip 0, clip 1} / += w.hi * ..: the weight pair is a 64-bit register pair as it lies in the image
__device__ __forceinline__ void pk_lo(f32x2& acc, f32x2 w, f32x2 x) { asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(w), "v"(x)); }
__device__ __forceinline__ void pk_hi(f32x2& acc, f32x2 w, f32x2 x) { asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(w), "v"(x)); }

// row_reduce_scatter4 for two clips: the same additions in the same order, the last level (the lane two further) keeps clip (ks >> 1) & 1
// instead of both: lanes 4 c, 4 c + 1 of the row end with column c's total of clip 0, lanes 4 c + 2, 4 c + 3 with clip 1's
__device__ __forceinline__ float row_reduce_scatter4_pair(const float (&a)[4], const float (&b)[4], int ks) {
  const bool hi = (ks & 8) != 0, q4 = (ks & 4) != 0, b1 = (ks & 2) != 0;
  float ta0 = hi ? a[2] : a[0], ta1 = hi ? a[3] : a[1], tb0 = hi ? b[2] : b[0], tb1 = hi ? b[3] : b[1];
  ta0 += dpp_mirror(hi ? a[0] : a[2]);
  ta1 += dpp_mirror(hi ? a[1] : a[3]);
  tb0 += dpp_mirror(hi ? b[0] : b[2]);
  tb1 += dpp_mirror(hi ? b[1] : b[3]);
  float wa = q4 ? ta1 : ta0, wb = q4 ? tb1 : tb0;
  wa += dpp_half_mirror(q4 ? ta0 : ta1);
  wb += dpp_half_mirror(q4 ? tb0 : tb1);
  wa += dpp_xor1(wa);
  wb += dpp_xor1(wb);
  return (b1 ? wb : wa) + dpp_xor2(b1 ? wa : wb);
}
// row_reduce_scatter2 for two clips: lanes 0-7 of the row column 0, lanes 8-15 column 1; inside every quad lanes 0, 1 clip 0, lanes 2, 3 clip 1
__device__ __forceinline__ float row_reduce_scatter2_pair(float a0, float a1, float b0, float b1v, int ks) {
  const bool hi = (ks & 8) != 0, b1 = (ks & 2) != 0;
  float ta = (hi ? a1 : a0) + dpp_mirror(hi ? a0 : a1);
  float tb = (hi ? b1v : b0) + dpp_mirror(hi ? b0 : b1v);
  ta += dpp_half_mirror(ta);
  tb += dpp_half_mirror(tb);
  ta += dpp_xor1(ta);
  tb += dpp_xor1(tb);
  return (b1 ? tb : ta) + dpp_xor2(b1 ? ta : tb);
}

// timing builds only (results wrong): 1 every bias product twice, 8 no look loads, 16 no row loads, 32 the rows' buffer is not waited for,
// 64 the row loads go into registers nobody reads and are never waited for by their data
#ifndef MMK_SP_PAIR_TIMING
#define MMK_SP_PAIR_TIMING 0
#endif
constexpr int kPairTripVisits = 40;   // fewer visits per step than this: the step is one visit's trip round the ring, and nobody pauses between two looks (as the one-clip form below 40 clips)
__device__ __forceinline__ bool chain_wait2(const Lds2& S, int q, unsigned v, bool nap, int32_t* err) {
  unsigned spins = 0;
  if (!nap) {      // (the trip-bound regime: the bias first - it is there a step ahead -, then ONE counter in the six-instruction loop of chain_wait)
    while (__hip_atomic_load(&S.ready[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < 2 * v + 2) {
      if (++spins > kSpinLimit || ((spins & 4095u) == 0 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
        atomicExch(err, 1);
        return false;
      }
    }
    if (__builtin_expect(lds_spin_ge(&S.arrived[v & 3], v + 1) < v + 1, 0)) {
      atomicExch(err, 1);
      return false;
    }
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    return true;
  }
  for (;;) {
    const unsigned arr = __hip_atomic_load(&S.arrived[v & 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const unsigned rd = __hip_atomic_load(&S.ready[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (arr >= v + 1 && rd >= 2 * v + 2) break;
    if (kChainSleep > 0 && nap) __builtin_amdgcn_s_sleep(kChainSleep);
    if (++spins > kSpinLimit || ((spins & 4095u) == 0 && __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
      atomicExch(err, 1);
      return false;
    }
  }
  __atomic_signal_fence(__ATOMIC_SEQ_CST);
  return true;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// chain waves, two clips per visit: lane l ends with gate row l / 4 and residual channel l / 8 of the wave for clip (l / 2) & 1
// ------------------------------------------------------------------------------------------------------------------------------------
__device__ void chain_role2(const WnSpipeArgs& a, Lds2& S, int stage, int p, int q, int lane) {
  const int W = 4 * p + q;
  const int ks = lane & 15;
  const int j = lane >> 2, j8 = lane >> 3;
  const int clip = (lane >> 1) & 1;
  f32x4s wz[32], wr[8], wh[4];
  {
    const f32x4s* img = reinterpret_cast<const f32x4s*>(a.img_chain) + ((int64_t)stage * kWavesPerStage + W) * kChainRegs * 64 + lane;
#pragma unroll
    for (int i = 0; i < 32; ++i) wz[i] = img[i * 64];
#pragma unroll
    for (int i = 0; i < 8; ++i) wr[i] = img[(32 + i) * 64];
#pragma unroll
    for (int i = 0; i < 4; ++i) wh[i] = img[(40 + i) * 64];
  }
  float bx = a.cst_chain[((int64_t)stage * kWavesPerStage + W) * 64 + lane];
  // (in their registers before the visit loop: see chain_role)
#pragma unroll
  for (int i = 0; i < 32; ++i) asm volatile("" : "+v"(wz[i]));
#pragma unroll
  for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(wr[i]));
#pragma unroll
  for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(wh[i]));
  asm volatile("" : "+v"(bx));
  const int64_t hid_words = (int64_t)a.Bmax * kSpSlots * kH1;
  const int grp = stage >> 2;
  const bool hid_chain_in = stage >= 2 && ((stage - 1) >> 2) == grp;
  const bool hid_last = stage == a.L - 1 || ((stage + 1) >> 2) != grp;
  const bool hid_local = hid_last ? grp == (a.L >> 2) : true;
  unsigned* hid_out = (hid_last ? a.hidgrp + (int64_t)grp * hid_words : a.hidmsg + (int64_t)(stage + 1) * hid_words) + 4 * W + (lane >> 4);
  const bool g_row = (j & 1) != 0;
  const float gate_scale = g_row ? -1.4426950408889634f : -2.8853900817779268f;
  const float gate_k = g_row ? 1.f : 2.f, gate_shift = g_row ? 0.f : -1.f;
  const bool local_next = ((stage + 1) >> 2) == (stage >> 2);
  const int64_t stage_words = (int64_t)a.Bmax * kSpSlots * kMsgFloats;
  unsigned* msg_out = a.msg + (int64_t)(stage + 1) * stage_words;
  const int kso = ((lane & 16) ? kHalf2 : 0) + ks * kSlice2;          // K slice lane & 31 of 16 channels: x in the even rows of 16 lanes, y in the odd ones
  const int yr_off = kHalf2 + ks * kSlice2;                           // y[16 ks ..]
  const int xin_off = pad2_of(8 * W + j8) + clip;
  const bool pub_lane = (lane & 7) < 4;                               // per channel: x and y of clip 0, x and y of clip 1
  const int pub_off = W * 16 + (lane & 1) * 8 + (lane >> 3);
  const int ring_mask = a.ring[stage] - 1;
  float* hist = a.hist[stage];
  const int64_t slot_stride = (int64_t)a.Bmax * kC;
  const int V = a.B >> 1, n_steps = (int)a.n_steps, Bcap = bias_cap(a.B);
  const bool nap = V >= kPairTripVisits;
  unsigned v = 0;
  for (int s = 0; s < n_steps; ++s) {
    const int64_t tau = a.t0 - 1 + s;
    const int slot = s & 3, pslot = (s + 2) & 3;
    for (int cv = 0; cv < V; ++cv, ++v) {
      if (!chain_wait2(S, q, v, nap, a.err_flag)) return;
      __builtin_amdgcn_s_setprio(kChainPrio);
      if (MMK_SP_ABL & 16) {          // (timing builds only: the chain waves do nothing)
        lds_signal(&S.hdone[q], v + 1, lane);
        continue;
      }
      const int cm = 2 * cv + clip;                                   // this lane's clip
      const float bzv = S.bias[bias_off(q, s & 1, cm, j, Bcap)];
      const float* xb = S.xy[v & (kXyRing - 1)];
      // ---- z = [W1 | W1 R] . [x ; y] of both clips: 8 gate rows x ONE K slice of 16 per lane, 8 reads of 2 channels x 2 clips, 128 packed FMAs ----
      f32x2 acc[8];
#pragma unroll
      for (int cc = 0; cc < 8; ++cc) acc[cc] = f32x2{0.f, 0.f};
      f32x2 rac[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};
      float xin;
      if (!nap) {      // (the rolling window where the step is one visit's trip: 64 clips -1 %; at a stage's beat it costs 1 %: 128 clips)
        // The 16 reads of a visit's products in a rolling window of four: reads k + 2 and k + 3 go out when the products of read pair k are through - left to the compiler,
        // the next pair went out behind the products of TWO pairs (it re-uses their registers) and was waited for at once: an LDS round trip three times per visit.
        // Pairs 0 - 3: the gate products' K slice; pairs 4 - 7: the y slice of the residual product.
        f32x4s ra[2], rc[2];
        auto rd = [&](int k, int b) {
          const float* src = k < 4 ? xb + kso + 8 * k : xb + yr_off + 8 * (k - 4);
          ra[b] = *reinterpret_cast<const f32x4s*>(src);
          rc[b] = *reinterpret_cast<const f32x4s*>(src + 4);
        };
        rd(0, 0);
        rd(1, 1);
        xin = xb[xin_off];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const f32x4s xa = ra[k & 1], xc = rc[k & 1];
          if (k < 4) {
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
              const f32x4s wq = wz[cc * 4 + k];
              pk_lo(acc[cc], f32x2{wq[0], wq[1]}, f32x2{xa[0], xa[1]});
              pk_hi(acc[cc], f32x2{wq[0], wq[1]}, f32x2{xa[2], xa[3]});
              pk_lo(acc[cc], f32x2{wq[2], wq[3]}, f32x2{xc[0], xc[1]});
              pk_hi(acc[cc], f32x2{wq[2], wq[3]}, f32x2{xc[2], xc[3]});
            }
          } else {
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
              const f32x4s wq = wr[cc * 4 + (k - 4)];
              pk_lo(rac[cc], f32x2{wq[0], wq[1]}, f32x2{xa[0], xa[1]});
              pk_hi(rac[cc], f32x2{wq[0], wq[1]}, f32x2{xa[2], xa[3]});
              pk_lo(rac[cc], f32x2{wq[2], wq[3]}, f32x2{xc[0], xc[1]});
              pk_hi(rac[cc], f32x2{wq[2], wq[3]}, f32x2{xc[2], xc[3]});
            }
          }
          __builtin_amdgcn_sched_barrier(0);
          if (k + 2 < 8) rd(k + 2, k & 1);
          __builtin_amdgcn_sched_barrier(0);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4s xa = *reinterpret_cast<const f32x4s*>(xb + kso + 8 * i), xc = *reinterpret_cast<const f32x4s*>(xb + kso + 8 * i + 4);
#pragma unroll
          for (int cc = 0; cc < 8; ++cc) {
            const f32x4s wq = wz[cc * 4 + i];
            pk_lo(acc[cc], f32x2{wq[0], wq[1]}, f32x2{xa[0], xa[1]});
            pk_hi(acc[cc], f32x2{wq[0], wq[1]}, f32x2{xa[2], xa[3]});
            pk_lo(acc[cc], f32x2{wq[2], wq[3]}, f32x2{xc[0], xc[1]});
            pk_hi(acc[cc], f32x2{wq[2], wq[3]}, f32x2{xc[2], xc[3]});
          }
        }
        // ---- the layer's own input x_s = x_{s-1} + (R y + br): 2 channels x 16 inputs per lane, both clips ----------------------------------
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4s ya = *reinterpret_cast<const f32x4s*>(xb + yr_off + 8 * i), yc = *reinterpret_cast<const f32x4s*>(xb + yr_off + 8 * i + 4);
#pragma unroll
          for (int cc = 0; cc < 2; ++cc) {
            const f32x4s wq = wr[cc * 4 + i];
            pk_lo(rac[cc], f32x2{wq[0], wq[1]}, f32x2{ya[0], ya[1]});
            pk_hi(rac[cc], f32x2{wq[0], wq[1]}, f32x2{ya[2], ya[3]});
            pk_lo(rac[cc], f32x2{wq[2], wq[3]}, f32x2{yc[0], yc[1]});
            pk_hi(rac[cc], f32x2{wq[2], wq[3]}, f32x2{yc[2], yc[3]});
          }
        }
        xin = xb[xin_off];
      }
      // the two rows of 16 lanes that hold the same 8 gate rows swap halves (even rows keep gate rows 0-3, odd rows 4-7), per clip
      float zc0[4], zc1[4];
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const auto s0 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[cc][0]), __float_as_uint(acc[4 + cc][0]), false, false);
        const auto s1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[cc][1]), __float_as_uint(acc[4 + cc][1]), false, false);
        zc0[cc] = __uint_as_float(s0[0]) + __uint_as_float(s0[1]);
        zc1[cc] = __uint_as_float(s1[0]) + __uint_as_float(s1[1]);
      }
      float z = row_reduce_scatter4_pair(zc0, zc1, ks);
      const float xs = row_reduce_scatter2_pair(rac[0][0], rac[1][0], rac[0][1], rac[1][1], ks);
      const float xnew = xin + (xs + bx);
      z += bzv;
      // tanh(f) sigmoid(g) (wavenet_v2.py:151); the g row sits four lanes up (same clip)
      const float act = fmaf(mmk_rcp(1.0f + __builtin_amdgcn_exp2f(z * gate_scale)), gate_k, gate_shift);
      const float other = dpp_move<dpp_row_shl(4)>(act);   // row_shl:4
      const float y = act * other;
      // ---- publish 8 x | 8 y per clip, re-poison the same words two steps ahead, keep x_s for the delayed taps --------------------------------
      unsigned* dst = msg_out + ((int64_t)cm * kSpSlots + slot) * kMsgFloats + pub_off;
      if (pub_lane) msg_store(dst, msg_bits((lane & 1) ? y : xnew), local_next);
#ifdef MMK_DIAG
      // diagnostic build: wall clock (100 MHz) of every visit's publish in the launch's middle step, per stage (the plan prints publish -> seen -> publish)
      if (a.stamps && s == n_steps / 2 && p == 0 && q == 0 && lane == 0 && cv < 32) a.stamps[256 + stage * 32 + cv] = __builtin_amdgcn_s_memrealtime();
      if (a.stamps && s == n_steps / 2 && cv == 5 && q == 0 && lane == 0) a.stamps[256 + 2048 + stage * 8 + p] = __builtin_amdgcn_s_memrealtime();      // every CU of the stage, visit 5
#endif
      __builtin_amdgcn_s_setprio(0);
      if (pub_lane) msg_store(msg_out + ((int64_t)cm * kSpSlots + pslot) * kMsgFloats + pub_off, kSpPoison, local_next);
      if ((lane & 5) == 0) hist[(tau & ring_mask) * slot_stride + (int64_t)cm * kC + 8 * W + j8] = xnew;
      // ---- the hidden units' sum, handed on (both clips) -----------------------------------------------------------------------------------------
      if (stage >= 1) {
        f32x2 hc[2] = {f32x2{0.f, 0.f}, f32x2{0.f, 0.f}};
        if (!(MMK_SP_ABL & 128))
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const f32x4s ya = *reinterpret_cast<const f32x4s*>(xb + yr_off + 8 * i), yc = *reinterpret_cast<const f32x4s*>(xb + yr_off + 8 * i + 4);
          pk_lo(hc[0], f32x2{wh[i][0], wh[i][1]}, f32x2{ya[0], ya[1]});
          pk_hi(hc[1], f32x2{wh[i][0], wh[i][1]}, f32x2{ya[2], ya[3]});
          pk_lo(hc[0], f32x2{wh[i][2], wh[i][3]}, f32x2{yc[0], yc[1]});
          pk_hi(hc[1], f32x2{wh[i][2], wh[i][3]}, f32x2{yc[2], yc[3]});
        }
        const f32x2 hsum = hc[0] + hc[1];
        const float hs0 = row_sum(hsum[0]);
        const float hs1 = row_sum(hsum[1]);
        float hin = 0.f;
        if (hid_chain_in && !(MMK_SP_ABL & 256)) {
          if (!lds_wait1(&S.hidin_ready[v & 3], v + 1, a.err_flag)) return;
          hin = S.hidin[v & (kXyRing - 1)][ks & 1][4 * q + (lane >> 4)];
        }
        if (ks < 2) {        // lane 0 of the row: clip 0's sum, lane 1: clip 1's
          msg_store(hid_out + ((int64_t)(2 * cv + ks) * kSpSlots + slot) * kH1, msg_bits(hin + (ks ? hs1 : hs0)), hid_local);
          msg_store(hid_out + ((int64_t)(2 * cv + ks) * kSpSlots + pslot) * kH1, kSpPoison, hid_local);
        }
      }
      lds_signal(&S.hdone[q], v + 1, lane);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------------------
// helper waves, two clips per visit.  The loop of helper_role in its four-behind form (LAG4, biases on the matrix pipe), counted in
// visits of two clips: V = B / 2 visits per step; rows and biases are kept in CLIP-visits (step * B + clip), a batch of four of them = two visits
// ------------------------------------------------------------------------------------------------------------------------------------
__device__ void helper_role2(const WnSpipeArgs& a, Lds2& S, int stage, int p, int h, int lane) {
  const int W = 4 * p + h;
  f32x4s w0[16], wc[16];
  {
    // the helper image in the matrix operand's order: register m (e = 0 .. 3) = W[row 4 g + i][half 256 + 16 (m & 15) + 4 ksub + e]
    const f32x4s* img = reinterpret_cast<const f32x4s*>(a.img_helper) + ((int64_t)stage * kWavesPerStage + W) * kHelperRegs * 64;
    const int g = (lane >> 2) & 3, i = lane & 3, ksub = lane >> 4;
#pragma unroll
    for (int m = 0; m < 16; ++m) w0[m] = img[(i * 4 + ksub) * 64 + 16 * g + m];
#pragma unroll
    for (int m = 0; m < 16; ++m) wc[m] = img[(16 + i * 4 + ksub) * 64 + 16 * g + m];
  }
  f32x4s bz4;
  {
    const float* cst = a.cst_helper + ((int64_t)stage * kWavesPerStage + W) * 64 + 16 * ((lane >> 2) & 3);
    bz4 = f32x4s{cst[0], cst[4], cst[8], cst[12]};
    asm volatile("" : "+v"(bz4));
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(w0[i]));
#pragma unroll
  for (int i = 0; i < 16; ++i) asm volatile("" : "+v"(wc[i]));
  const int d = a.dil[stage], ring_mask = a.ring[stage] - 1;
  const int64_t slot_stride = (int64_t)a.Bmax * kC;
  const int64_t stage_words = (int64_t)a.Bmax * kSpSlots * kMsgFloats;
  const int B = a.B, Bcap = bias_cap(a.B), V = a.B >> 1;
  const int n_vis = (int)a.n_steps * V, n_cv = (int)a.n_steps * B;
  const int64_t hid_words = (int64_t)a.Bmax * kSpSlots * kH1;
  const bool hid_chain_in = stage >= 2 && ((stage - 1) >> 2) == (stage >> 2);
  const bool nap = V >= kPairTripVisits;
  const int roff = V - 1;                       // the rows of visit it + roff are asked for in iteration it (by the helper on duty) and staged in its next duty, it + 4
  const __amdgpu_buffer_rsrc_t inbox = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned*>(a.msg + (int64_t)stage * stage_words), 0, -1, 0x00020000);
  const int look_off = 32 * lane;
  const int st_off = ((lane & 1) ? kHalf2 : 0) + pad2_of(8 * (lane >> 1));
  // the two messages of a visit (clips 2 cv, 2 cv + 1): 32 bytes per lane and clip, past this CU's L1 (sc1)
  auto look2 = [&](int cv, int slot, u32x4s (&m)[4]) {
    asm volatile("" ::: "memory");
    if (MMK_SP_PAIR_TIMING & 8) { m[0] = m[1] = m[2] = m[3] = u32x4s{0, 0, 0, 0}; return; }      // (timing builds only: no look loads)
    const int off = ((2 * cv * kSpSlots + slot) * kMsgFloats) * 4 + look_off;
    m[0] = __builtin_amdgcn_raw_buffer_load_b128(inbox, off, 0, 16);
    m[1] = __builtin_amdgcn_raw_buffer_load_b128(inbox, off + 16, 0, 16);
    m[2] = __builtin_amdgcn_raw_buffer_load_b128(inbox, off + kSpSlots * kMsgFloats * 4, 0, 16);
    m[3] = __builtin_amdgcn_raw_buffer_load_b128(inbox, off + kSpSlots * kMsgFloats * 4 + 16, 0, 16);
  };
  const bool freerun = (MMK_SP_ABL & 4) != 0;
  auto landed2 = [&](const u32x4s (&m)[4]) {
    if (freerun) return true;
    unsigned mx = 0;      // (the poison word is the largest unsigned: one maximum of the 16 words, one compare)
#pragma unroll
    for (int k = 0; k < 4; ++k) mx = max(max(mx, max(m[k][0], m[k][1])), max(m[k][2], m[k][3]));
    return __all(mx != kSpPoison) != 0;
  };
  const __amdgpu_buffer_rsrc_t ring = __builtin_amdgcn_make_buffer_rsrc(a.hist[stage], 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t own = __builtin_amdgcn_make_buffer_rsrc(a.msg + (int64_t)(stage + 1) * stage_words, 0, -1, 0x00020000);
  const bool cond_lane = 4 * lane < a.C1;
  // the rows of the bias of clip-visit (c2, s2): see helper_role
  auto request_rows = [&](int s2, int c2, bool from_own, u32x4s& xr, f32x4s& cr, bool with_cond = true) {
    if (MMK_SP_PAIR_TIMING & 16) { xr = u32x4s{0, 0, 0, 0}; cr = f32x4s{0.f, 0.f, 0.f, 0.f}; return; }      // (timing builds only: no row loads)
    if (MMK_SP_PAIR_TIMING & 64) {      // (timing builds only: the loads go out - into registers nobody reads - and are never waited for by their data)
      const int64_t tp = a.t0 - 1 + s2 - d;
      const float* rp = a.hist[stage] + ((tp < 0 ? 0 : (tp & ring_mask)) * slot_stride + (int64_t)c2 * kC + 4 * lane);
      const float* cp = a.cproj + ((int64_t)c2 * a.cond_steps + s2) * a.C1 + 4 * (cond_lane ? lane : 0);
      asm volatile("global_load_dwordx4 v[248:251], %0, off sc1\n\tglobal_load_dwordx4 v[252:255], %1, off" :: "v"(rp), "v"(cp) : "v248", "v249", "v250", "v251", "v252", "v253", "v254", "v255");
      xr = u32x4s{0, 0, 0, 0}; cr = f32x4s{0.f, 0.f, 0.f, 0.f};
      return;
    }
    if (from_own) {
      const int off = (((c2 * kSpSlots + ((s2 - 1) & 3)) * kMsgFloats) + (lane >> 1) * 16 + (lane & 1) * 4) * 4;
      xr = __builtin_amdgcn_raw_buffer_load_b128(own, off, 0, 16);
    } else {
      const int64_t tp = a.t0 - 1 + s2 - d;
      if (tp >= 0) xr = __builtin_amdgcn_raw_buffer_load_b128(ring, (int)(((tp & ring_mask) * slot_stride + (int64_t)c2 * kC + 4 * lane) * 4), 0, 16);
      else xr = u32x4s{0, 0, 0, 0};
    }
    if (!with_cond) return;
    if (cond_lane && !(MMK_SP_ABL & 1)) cr = *reinterpret_cast<const f32x4s*>(a.cproj + ((int64_t)c2 * a.cond_steps + s2) * a.C1 + 4 * lane);
    else cr = f32x4s{0.f, 0.f, 0.f, 0.f};
  };
  // into the batch's buffer, once every helper is through with the batch that used it before
  auto stage_rows = [&](unsigned cvv, const u32x4s& xr, const f32x4s& cr) -> bool {
    const unsigned kb = cvv >> 2;
    if (!(MMK_SP_PAIR_TIMING & 32))      // (timing builds only: the rows' buffer is not waited for)
    if (kb >= (unsigned)kRowsbDepth && !lds_wait4(S.ready, 4 * (kb - kRowsbDepth) + 4, a.err_flag)) return false;
    float* dst = &S.rowsb[kb & (kRowsbDepth - 1)][cvv & 3][4 * lane];
    *reinterpret_cast<f32x4s*>(dst) = f32x4s{__uint_as_float(xr[0]), __uint_as_float(xr[1]), __uint_as_float(xr[2]), __uint_as_float(xr[3])};
    *reinterpret_cast<f32x4s*>(dst + 256) = cr;
    lds_signal(&S.rows_ready[cvv & 7], cvv + 1, lane);
    return true;
  };
  // a quarter of batch kb's products (see helper_role): clip-visits in [v_lo, v_hi) exist
  f32x4s macc[4] = {f32x4s{0.f, 0.f, 0.f, 0.f}, f32x4s{0.f, 0.f, 0.f, 0.f}, f32x4s{0.f, 0.f, 0.f, 0.f}, f32x4s{0.f, 0.f, 0.f, 0.f}};
  auto mf_chunk = [&](int kb, int ch, int v_lo, int v_hi) -> bool {
    if (ch == 0) {
      const int vv = 4 * kb + (lane & 3);
      const bool need = vv >= v_lo && vv < v_hi;
      unsigned spins = 0;
      while (!__all(!need || __hip_atomic_load(&S.rows_ready[vv & 7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= (unsigned)vv + 1)) {
        if (kLdsSleep > 0) __builtin_amdgcn_s_sleep(kLdsSleep);
        if (++spins > kSpinLimit || ((spins & 4095u) == 0 && __hip_atomic_load(a.err_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
          atomicExch(a.err_flag, 1);
          return false;
        }
      }
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
#pragma unroll
      for (int e = 0; e < 4; ++e) macc[e] = f32x4s{0.f, 0.f, 0.f, 0.f};
    }
    auto products = [&](auto chc) {
      constexpr int CH = decltype(chc)::value;
      const float* xb = &S.rowsb[kb & (kRowsbDepth - 1)][lane & 3][(CH >> 1) * 256 + 4 * (lane >> 4)];
      constexpr int m0 = (CH & 1) * 8;
      // (all eight reads of the chunk first: with a read two products ahead of its use the chunk starts with a full LDS round trip in front of its first product)
      f32x4s xv[8];
#pragma unroll
      for (int mm = 0; mm < 8; ++mm) xv[mm] = *reinterpret_cast<const f32x4s*>(xb + 16 * (m0 + mm));
#pragma unroll
      for (int mm = 0; mm < 8; ++mm) {
        const f32x4s wv = (CH >> 1) ? wc[m0 + mm] : w0[m0 + mm];
#pragma unroll
        for (int e = 0; e < 4; ++e) macc[e] = __builtin_amdgcn_mfma_f32_4x4x1f32(wv[e], xv[mm][e], macc[e], 0, 0, 0);
      }
    };
    if (!(MMK_SP_ABL & 8))
    for (int rep = 0; rep < ((MMK_SP_PAIR_TIMING & 1) ? 2 : 1); ++rep)      // (timing builds only: every product twice)
    switch (ch) {
      case 0: products(std::integral_constant<int, 0>{}); break;
      case 1: products(std::integral_constant<int, 1>{}); break;
      case 2: if (a.C1 > 0) products(std::integral_constant<int, 2>{}); break;
      default: if (a.C1 > 0) products(std::integral_constant<int, 3>{}); break;
    }
    if (ch == 3) {
      f32x4s tot;
      const f32x4s msum = (macc[0] + macc[1]) + (macc[2] + macc[3]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const auto s16 = __builtin_amdgcn_permlane16_swap(__float_as_uint(msum[r]), __float_as_uint(msum[r]), false, false);
        const float y = __uint_as_float(s16[0]) + __uint_as_float(s16[1]);
        const auto s32 = __builtin_amdgcn_permlane32_swap(__float_as_uint(y), __float_as_uint(y), false, false);
        tot[r] = __uint_as_float(s32[0]) + __uint_as_float(s32[1]);
      }
      const int vv = 4 * kb + (lane & 3);
      if (lane < 16 && vv >= v_lo && vv < v_hi) {
        const int s2 = vv / B, c2 = vv - s2 * B;
        *reinterpret_cast<f32x4s*>(&S.bias[bias_off(h, s2 & 1, c2, 4 * (lane >> 2), Bcap)]) = tot + bz4;
      }
      lds_signal(&S.ready[h], (unsigned)(4 * kb + 4 < v_hi ? 4 * kb + 4 : v_hi), lane);
    }
    return true;
  };
  u32x4s xr0 = u32x4s{0, 0, 0, 0}, xr1 = u32x4s{0, 0, 0, 0};
  f32x4s cr0 = f32x4s{0.f, 0.f, 0.f, 0.f}, cr1 = f32x4s{0.f, 0.f, 0.f, 0.f};
  // ---- step 0: the rows the warm-up wrote -----------------------------------------------------------------------------------------------------
  for (int kb = 0; 4 * kb < B; ++kb) {
    if (4 * kb + h < B) {      // (an even clip count that is no multiple of 4: the step's last batch holds two clips of this step and the first two of the next)
      request_rows(0, 4 * kb + h, false, xr0, cr0);
      if (!stage_rows((unsigned)(4 * kb + h), xr0, cr0)) return;
    }
    for (int ch = 0; ch < 4; ++ch)
      if (!mf_chunk(kb, ch, 0, B)) return;
  }
  int s = 0, cv = 0;                              // visit it = (cv, s)
  int su = 0, cu = V - 5;                         // visit it + V - 5 = (cu, su): its rows are staged in iteration it
  int sa = roff / V, ca = roff % V;               // visit it + roff: the rows asked for in iteration it
  int sl = 4 / V, cl = 4 % V;                     // visit it + 4: the messages whose first look goes out in iteration it
  u32x4s m[4];
  bool staged_next = false;
  // the hidden units' hand-over of a visit is asked for together with the FIRST look at its messages (four visits ahead): where the clips queue up it is there
  // when the messages are staged - asked for at the staging it was a round trip per duty in front of everything the four helpers do in lock step (the beat, 96+ clips)
  const unsigned* hid_base = a.hidmsg + (int64_t)stage * hid_words + 16 * p + (lane & 15);
  unsigned hid_pre = kSpPoison;
  auto pre_ask_hid = [&](int cc, int ss) {
    if (hid_chain_in && !(MMK_SP_ABL & 32)) hid_pre = msg_load(hid_base + ((int64_t)(2 * cc + ((lane >> 4) & 1)) * kSpSlots + (ss & 3)) * kH1);
  };
  if (h < n_vis) { look2(h % V, (h / V) & 3, m); pre_ask_hid(h % V, h / V); }
  else m[0][0] = kSpPoison;
  // the hidden units' hand-over of the stage below for a staged visit: asked for right behind the staging, taken at the END of the iteration (the
  // stage below hands it on behind its publish, the chain waves here need it behind theirs: a round trip that nothing has to wait for)
  int hid_vv = -1;
  const unsigned* hid_src = nullptr;
  unsigned hid_w = 0;
  auto ask_hid = [&](int vv, int cc, int ss) {
    if (!hid_chain_in) return;
    if (MMK_SP_ABL & 32) {
      lds_signal(&S.hidin_ready[vv & 3], (unsigned)vv + 1, lane);
      return;
    }
    // lanes 0-15: clip 2 cc, lanes 16-31: clip 2 cc + 1 (the upper half of the wave looks at the same words)
    hid_src = hid_base + ((int64_t)(2 * cc + ((lane >> 4) & 1)) * kSpSlots + (ss & 3)) * kH1;
    if (__all(hid_pre != kSpPoison)) {      // (asked for with the first look, and there)
      if (lane < 32) S.hidin[vv & (kXyRing - 1)][lane >> 4][lane & 15] = __uint_as_float(hid_pre);
      lds_signal(&S.hidin_ready[vv & 3], (unsigned)vv + 1, lane);
      hid_pre = kSpPoison;
      return;
    }
    hid_w = msg_load(hid_src);
    hid_vv = vv;
  };
  auto take_hid = [&]() -> bool {
    if (hid_vv < 0) return true;
    unsigned spins = 0;
    while (!__all(hid_w != kSpPoison) && !freerun) {
      if (++spins > kSpinLimit || ((spins & 1023u) == 0 && __hip_atomic_load(a.err_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
        atomicExch(a.err_flag, 1);
        return false;
      }
      hid_w = msg_load(hid_src);
    }
    if (lane < 32) S.hidin[hid_vv & (kXyRing - 1)][lane >> 4][lane & 15] = __uint_as_float(hid_w);
    lds_signal(&S.hidin_ready[hid_vv & 3], (unsigned)hid_vv + 1, lane);
    hid_vv = -1;
    return true;
  };
  // a landed pair of messages into the image of visit vv: per channel {clip 0, clip 1}
  auto stage_message = [&](int vv, const u32x4s (&mm)[4]) {
    float* dst = &S.xy[vv & (kXyRing - 1)][st_off];
    *reinterpret_cast<f32x4s*>(dst) = f32x4s{__uint_as_float(mm[0][0]), __uint_as_float(mm[2][0]), __uint_as_float(mm[0][1]), __uint_as_float(mm[2][1])};
    *reinterpret_cast<f32x4s*>(dst + 4) = f32x4s{__uint_as_float(mm[0][2]), __uint_as_float(mm[2][2]), __uint_as_float(mm[0][3]), __uint_as_float(mm[2][3])};
    *reinterpret_cast<f32x4s*>(dst + 8) = f32x4s{__uint_as_float(mm[1][0]), __uint_as_float(mm[3][0]), __uint_as_float(mm[1][1]), __uint_as_float(mm[3][1])};
    *reinterpret_cast<f32x4s*>(dst + 12) = f32x4s{__uint_as_float(mm[1][2]), __uint_as_float(mm[3][2]), __uint_as_float(mm[1][3]), __uint_as_float(mm[3][3])};
#if defined(MMK_DIAG) && !defined(MMK_SP_PAIR_STAMP_ANY)
    if (a.stamps && vv / V == (int)a.n_steps / 2 && p == 0 && lane == 0 && vv % V < 32) a.stamps[256 + 1024 + stage * 32 + vv % V] = __builtin_amdgcn_s_memrealtime();
#endif
    lds_signal(&S.arrived[vv & 3], (unsigned)vv + 1, lane);
    asm volatile("s_wakeup");
  };
  // look at the pair of messages of visit (cc, ss) until they are there, then stage them (the first look is in the registers already)
  auto await_and_stage = [&](int vv, int cc, int ss) -> bool {
    if (vv >= kXyRing - 2 && !lds_wait4(S.hdone, (unsigned)vv - (kXyRing - 2) + 1, a.err_flag)) return false;
    unsigned spins = 0;
#if defined(MMK_DIAG) && defined(MMK_SP_PAIR_STAMP_ANY)
    bool any_seen = false;      // (timing variant of the diagnostic build: the "seen" stamp is the first look that shows ANY word of the pair - the rest of publish -> seen is the producers' spread)
#endif
    while (!landed2(m)) {
#if defined(MMK_DIAG) && defined(MMK_SP_PAIR_STAMP_ANY)
      if (!any_seen) {
        bool some = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) some = some || m[k][0] != kSpPoison || m[k][1] != kSpPoison || m[k][2] != kSpPoison || m[k][3] != kSpPoison;
        if (__any(some)) {
          any_seen = true;
          if (a.stamps && vv / V == (int)a.n_steps / 2 && p == 0 && lane == 0 && vv % V < 32) a.stamps[256 + 1024 + stage * 32 + vv % V] = __builtin_amdgcn_s_memrealtime();
        }
      }
#endif
      if (++spins > kSpinLimit) {      // (one exit besides the messages: see helper_role)
        atomicExch(a.err_flag, 1);
        return false;
      }
      if (kPollGap > 0 && nap && spins > 1) __builtin_amdgcn_s_sleep(kPollGap);
      look2(cc, ss & 3, m);
    }
#if defined(MMK_DIAG) && defined(MMK_SP_PAIR_STAMP_ANY)
    if (!any_seen && a.stamps && vv / V == (int)a.n_steps / 2 && p == 0 && lane == 0 && vv % V < 32) a.stamps[256 + 1024 + stage * 32 + vv % V] = __builtin_amdgcn_s_memrealtime();
#endif
    stage_message(vv, m);
    ask_hid(vv, cc, ss);
    return true;
  };
  for (int it = 0; it < n_vis; ++it) {
    const bool duty = (it & 3) == h;
    // The rows are asked for and staged by the helper whose look duty was the visit BEFORE, not by the helper on look duty.  The registers
    // a row is loaded into live across four iterations, so the compiler waits for them - and before they are overwritten - with a count of ZERO: behind every load
    // the wave has in flight.  On the look-duty helper that was the first look at the messages of visit it + 4, sent out a moment before: a full round trip per
    // visit in front of what the four helpers do in lock step.  One iteration later that look has long come back.
    const bool rowduty = ((it - 1) & 3) == h;
    // ---- 1. the visit's messages --------------------------------------------------------------------------------------------------------------
    if (duty) {
      if (!staged_next && !await_and_stage(it, cv, s)) return;
      staged_next = false;
    }
    // ---- 2. the rows of visit it + V - 5, asked for in my last duty iteration - BEFORE the first look at the messages of visit it + 4 goes out: the rows' registers
    //      are waited for with a count of zero (the loop's loads are not countable at compile time), i.e. behind every load in flight - with the look in front of it
    //      that wait was a full round trip of the look, once per visit, in front of everything the four helpers do in lock step (helpers alone, 128 clips: 88 -> 67 us
    //      per step without the rows' loads)
    if (rowduty && it >= 5 && it + V - 5 < n_vis) {
      const unsigned u = (unsigned)(it + V - 5);
      if (d == 1) {
        unsigned spins = 0;
        while (!freerun && !__all(xr0[0] != kSpPoison && xr0[1] != kSpPoison && xr0[2] != kSpPoison && xr0[3] != kSpPoison && xr1[0] != kSpPoison &&
                                  xr1[1] != kSpPoison && xr1[2] != kSpPoison && xr1[3] != kSpPoison)) {
          if (++spins > kSpinLimit || ((spins & 1023u) == 0 && __hip_atomic_load(a.err_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
            atomicExch(a.err_flag, 1);
            return;
          }
          request_rows(su, 2 * cu, true, xr0, cr0, false);
          request_rows(su, 2 * cu + 1, true, xr1, cr1, false);
        }
      }
      if (!stage_rows(2 * u, xr0, cr0) || !stage_rows(2 * u + 1, xr1, cr1)) return;
    }
    if (duty) {
      if (it + 4 < n_vis) { look2(cl, sl & 3, m); pre_ask_hid(cl, sl); }
      else m[0][0] = kSpPoison;
    }
    // ---- my look duty is the NEXT visit: I look for those messages now and make this iteration's products afterwards (helper_role) ---------------
    if (((it + 1) & 3) == h && it + 1 < n_vis && !staged_next) {
      const int cn = cv + 1 == V ? 0 : cv + 1, sn = cv + 1 == V ? s + 1 : s;
      if (!await_and_stage(it + 1, cn, sn)) return;
      staged_next = true;
    }
    // ---- half a batch of biases: the batch before the one that visit it + V - 5 (staged in this iteration) belongs to ---------------------------
    {
      const int u = it + V - 5, kbc = (u >> 1) - 1;
      if (it >= 5 && kbc >= (B >> 2) && 4 * kbc < n_cv) {
        if (!mf_chunk(kbc, 2 * (u & 1), B, n_cv)) return;
        if (!mf_chunk(kbc, 2 * (u & 1) + 1, B, n_cv)) return;
      }
    }
    if (!take_hid()) return;
    // ---- 3. the rows of visit it + roff (the helper that looked: its next look duty is four visits away) ------------------------------------------
    if (rowduty && sa >= 1 && it + roff < n_vis) {
      request_rows(sa, 2 * ca, d == 1, xr0, cr0);
      request_rows(sa, 2 * ca + 1, d == 1, xr1, cr1);
    }
    if (++ca == V) { ca = 0; ++sa; }
    if (++cu == V) { cu = 0; ++su; }
    if (++cl == V) { cl = 0; ++sl; }
    if (++cv == V) { cv = 0; ++s; }
  }
}

__global__ __launch_bounds__(kThreads) void wavenet_spipe_pair_kernel(const WnSpipeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char spipe_lds2[];     // Lds2 + the bias image of bias_cap(B) clips
  Lds2& S = *reinterpret_cast<Lds2*>(spipe_lds2);
  __shared__ int s_role;
  const int tid = threadIdx.x;
  if (tid == 0) {      // roles from where the workgroup runs: see wavenet_spipe_kernel
    unsigned id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(id));
    id &= 0xf;
    const unsigned ticket = atomicAdd(a.xcd_count + (id & 7), 1u);
    int role = -1;
    if (id >= 8 || ticket >= 32) atomicExch(a.err_flag, 2);
    else role = (int)(id * 32 + ticket);
    s_role = role;
  }
  if (tid < 24) (&S.arrived[0])[tid] = 0;       // arrived, hdone, ready, hidin_ready, rows_ready are adjacent
  for (int i = tid; i < kRowsbDepth * 4 * kBRow; i += kThreads) (&S.rowsb[0][0][0])[i] = 0.f;      // (the conditioning columns above C1 are never written again)
  __syncthreads();
  const int role = s_role;
  if (role < 0) return;
  const int stage = role >> 3, p = role & 7;
  if (stage < 0 || stage > a.L) return;
  if (stage == a.L) {
    head_role<false>(a, p);
    return;
  }
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (wave < 4) chain_role2(a, S, stage, p, wave, lane);
  else helper_role2(a, S, stage, p, wave - 4, lane);
}
