// The body of k_w4_wgrad64h (kernels_w4_wgrad.hip has its description), included as TEXT into k_w4_wgrad64h and into the
// weight-gradient half of k_w4_gemm64h_wgrad64h.  In scope where it is included: the kernel's W4WgradHArgs `a` and W4_BLOCK, the
// workgroup's index in the weight gradient's own grid.  Text and not a device function: w4s_pass_body.inc has the reason.
  if (a.ctrl != nullptr && a.ctrl->done) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char wsm[];   // [W4WH_NST][V image 8 KB | Z image 8 KB]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int C = a.C, nRB = a.N >> 3, G16 = C >> 4, nCT = C >> 7, T = nCT * nCT;
  const int per_xcd = (36 * a.layers) >> 3;                       // (layer, component) pairs per XCD: 9 or 4.5 -> see the launcher
  const int xcd = W4_BLOCK & 7, slot = W4_BLOCK >> 3;
  const bool by_xcd = ((36 * a.layers) & 7) == 0;                 // (one layer -- the stem's: 36 pairs do not split over 8 XCDs: in order)
  const int pair = by_xcd ? xcd * per_xcd + slot / T : (int)W4_BLOCK / T, tile = by_xcd ? slot % T : (int)W4_BLOCK % T;
  const int layer = pair / 36, comp = pair - layer * 36;
  const int cit = tile / nCT, cot = tile - cit * nCT;
  const size_t cbytes = (size_t)nRB * G16 * 2048;                 // bytes per component
  const unsigned char* Vb = reinterpret_cast<const unsigned char*>(a.V[layer]) + comp * cbytes;
  const unsigned char* Zb = reinterpret_cast<const unsigned char*>(a.Z[layer]) + comp * cbytes;
  const float inv = ldexpf(1.f, -(*a.v_exp[layer] + *a.z_exp));

  // --- DMA roles: wave w brings instructions i = 4 w .. 4 w + 3 of a stage: i < 8 the V block g2l = i (lanes 0-31 part h, 32-63
  // part l), else the Z block g2l = i - 8.  Lane -> its 16-B chunk of the 512-B half part: LDS slot (s', hi, t) <- source (s' ^ odd, hi, t)
  const unsigned char* src[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = 4 * wave + k, isz = i >> 3, g2l = i & 7;
    const int part = lane >> 5, sg = lane & 31, ss = (sg >> 3) ^ (g2l & 1), hi = (sg >> 2) & 1, t = sg & 3;
    const int g2 = (isz ? cot : cit) * 8 + g2l;
    src[k] = (isz ? Zb : Vb) + ((size_t)g2 * 2 + part) * 1024 + ((ss * 2 + hi) * 4 + t) * 16;
  }
  const size_t rb_bytes = (size_t)G16 * 2048;
  const unsigned lds0 = (unsigned)(size_t)(w4_lds_ptr_t)wsm + (unsigned)(4 * wave) * 1024u;
  auto issue = [&](int q) {                                       // K step q = (row block q / 2, half q % 2)
    const size_t off = (size_t)(q >> 1) * rb_bytes + (size_t)(q & 1) * 512;
    const unsigned dst = lds0 + (unsigned)(q % W4WH_NST) * W4WH_STAGE;
#pragma unroll
    for (int k = 0; k < 4; ++k) w4wh_dma(src[k] + off, dst + (unsigned)k * 1024u);
  };
  // --- fragment reads (ds_read_b64_tr_b16): lane = (kh, g2a, m = 4 q4 + p): rows = tiles q4 of samples 2 kh, 2 kh + 1; 8-byte column quad p
  // = channels 4 p .. 4 p + 3 of its 16-channel block (hi = p & 1, gp = p >> 1); the lane receives channel m of the block
  const int wr = wave >> 1, wc = wave & 1;
  const int kh = lane >> 5, g2a = (lane >> 4) & 1, m = lane & 15, q4 = m >> 2, pq = m & 3;
  const int lane_off = (pq & 1) * 64 + q4 * 16 + (pq >> 1) * 8;
  const int s_lo = (2 * kh) ^ g2a, s_hi = (2 * kh + 1) ^ g2a;   // LDS slots of the two samples (odd blocks are stored swapped)
  auto frag = [&](const unsigned char* img, int g2l0, int part) -> w4_f16x8 {
    const unsigned char* pb = img + ((g2l0 + g2a) * 2 + part) * 512 + lane_off;
    const w4_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) w4_s16x4*)(pb + s_lo * 128));
    const w4_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) w4_s16x4*)(pb + s_hi * 128));
    const w4_s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(w4_f16x8, v);
  };
  float16_t acc[2][2];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[r][c][q] = 0.f;

  const int nK = 2 * nRB;
#pragma unroll
  for (int q = 0; q < W4WH_D; ++q)
    if (q < nK) issue(q);
  for (int q = 0; q < nK; ++q) {
    const int ahead = min(q + W4WH_D - 1, nK - 1) - q;          // stages issued behind stage q
    if (ahead >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (ahead == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // this wave's reads of stage q - 1 are in registers (its slot is refilled next)
    __builtin_amdgcn_s_barrier();
    if (q + W4WH_D < nK) issue(q + W4WH_D);
    const unsigned char* st = wsm + (q % W4WH_NST) * W4WH_STAGE;
    w4_f16x8 A[2][2], B[2][2];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int part = 0; part < 2; ++part) {
        A[r][part] = frag(st, 4 * wr + 2 * r, part);
        B[r][part] = frag(st + 8192, 4 * wc + 2 * r, part);
      }
#define W4WH_P(AP, BQ)                                                                       \
  _Pragma("unroll") for (int r = 0; r < 2; ++r) _Pragma("unroll") for (int c = 0; c < 2; ++c)  \
      acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[r][AP], B[c][BQ], acc[r][c], 0, 0, 0);
    W4WH_P(1, 0) W4WH_P(0, 1) W4WH_P(0, 0)   // smallest products first
#undef W4WH_P
  }
  // accumulator register q of a lane: row (q & 3) + 8 (q >> 2) + 4 kh = channel ci of the block, column lane & 31 = co
  float* o = a.dU + ((size_t)layer * 36 + comp) * C * C + (size_t)(cit * 128 + 64 * wr) * C + cot * 128 + 64 * wc + (lane & 31);
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = (q & 3) + 8 * (q >> 2) + 4 * kh;
        st_wt(o + (size_t)(32 * r + row) * C + 32 * c, acc[r][c][q] * inv);
      }
