// rectify_backward_pass.inc -- the one pass behind relu_backward_kernel and
// dropout_relu_backward_kernel (csr_ops.hip), included as text in both kernel bodies.
//
// As text and not as a __device__ __forceinline__ function: the compiler inlines such a callee
// after its first simplification passes, and the later passes then schedule every instantiation
// differently from the same statements written in the kernel (the gate kernel issued its
// gradient and gate loads one after the other instead of together: 0.97 against 0.73 ms at
// Twitter-World size, profiles/backward_once/). Included, the ten instantiations compile to the
// instruction streams they had as two pasted kernels.
//
// The including kernel has in scope: VEC (4: dwordx4 pieces, 1: dword), the kernel parameters
// M, K, rows_per_block, gY, ldg, g_out, ldo, partial, gate, ldgate, and
//   constexpr MaskSource kMask   where the rectify mask comes from (kMaskNone: g = t)
//   constexpr bool kDrop         t = keep ? gY * scale : 0 from the element's Philox word (row
//                                row0 + r, column c: one call per dwordx4 piece), else t = gY
//   Y, ldy                       read with kMaskY only
//   d, row0                      the DropKey and the logical row of row 0, read with kDrop only
// g = mask(t) is written to g_out (may alias gY) unless there is neither mask nor drop (column
// sums of gY only). Block = 4 waves; wave w takes rows r0 + w, r0 + w + 4, ...; lanes span the
// columns. Row blocks, wave interleave, accumulation order and the partial layout do not depend
// on kMask or kDrop, so the column sums are bitwise the same for the same g.
{
  constexpr bool kStore = kMask != kMaskNone || kDrop;
  __shared__ float red[4][kReluMaxK4 * 64 * 4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_block;
  const int64_t r1 = min(M, r0 + rows_per_block);
  const int pieces = (K + 64 * VEC - 1) / (64 * VEC);
  float acc[kReluMaxK4][VEC];
#pragma unroll
  for (int p = 0; p < kReluMaxK4; ++p)
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[p][e] = 0.f;
#pragma unroll 2
  for (int64_t r = r0 + w; r < r1; r += 4) {
    const float* gr = gY + r * ldg;
    const float* yr = kMask == kMaskY ? Y + r * ldy : nullptr;
    const uint8_t* gt = kMask == kMaskGate ? gate + r * ldgate : nullptr;
    float* orow = kStore ? g_out + r * ldo : nullptr;
    const int64_t i = row0 + r;
#pragma unroll
    for (int p = 0; p < kReluMaxK4; ++p) {
      if (p >= pieces) break;
      const int c = (p * 64 + lane) * VEC;
      if (c >= K) continue;
      if constexpr (VEC == 4) {
        const Philox4 pw = kDrop ? drop_words(d, i, c >> 2) : Philox4{};
        if (c + 4 > K) {  // ragged tail: element-wise, never touches columns >= K
          for (int e = 0; e < 4; ++e)
            if (c + e < K) {
              float o = gr[c + e];
              if constexpr (kDrop) o = drop_apply(d, pw.w[e], o);
              if constexpr (kMask == kMaskGate) o = gate_apply(o, gt[c + e]);
              else if constexpr (kMask == kMaskY) o = yr[c + e] > 0.f ? o : 0.f;
              if constexpr (kStore) orow[c + e] = o;
              acc[p][e] += o;
            }
          continue;
        }
        float4 o = *reinterpret_cast<const float4*>(gr + c);
        if constexpr (kDrop)
          o = make_float4(drop_apply(d, pw.w[0], o.x), drop_apply(d, pw.w[1], o.y),
                          drop_apply(d, pw.w[2], o.z), drop_apply(d, pw.w[3], o.w));
        if constexpr (kMask == kMaskGate) {
          const uint32_t gv = *reinterpret_cast<const uint32_t*>(gt + c);
          o = make_float4(gate_apply(o.x, gv & 0xffu), gate_apply(o.y, (gv >> 8) & 0xffu),
                          gate_apply(o.z, (gv >> 16) & 0xffu), gate_apply(o.w, gv >> 24));
        } else if constexpr (kMask == kMaskY) {
          const float4 yv = *reinterpret_cast<const float4*>(yr + c);
          o = make_float4(yv.x > 0.f ? o.x : 0.f, yv.y > 0.f ? o.y : 0.f,
                          yv.z > 0.f ? o.z : 0.f, yv.w > 0.f ? o.w : 0.f);
        }
        if constexpr (kStore) *reinterpret_cast<float4*>(orow + c) = o;
        acc[p][0] += o.x; acc[p][1] += o.y; acc[p][2] += o.z; acc[p][3] += o.w;
      } else {
        float o = gr[c];
        if constexpr (kDrop) o = drop_element(d, i, c, o);
        if constexpr (kMask == kMaskGate) o = gate_apply(o, gt[c]);
        else if constexpr (kMask == kMaskY) o = yr[c] > 0.f ? o : 0.f;
        if constexpr (kStore) orow[c] = o;
        acc[p][0] += o;
      }
    }
  }
  // combine the 4 waves (fixed order), one partial row per block
#pragma unroll
  for (int p = 0; p < kReluMaxK4; ++p)
#pragma unroll
    for (int e = 0; e < VEC; ++e) red[w][(p * 64 + lane) * VEC + e] = acc[p][e];
  __syncthreads();
  for (int c = threadIdx.x; c < K; c += 256) {
    const float v = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
    partial[static_cast<int64_t>(blockIdx.x) * K + c] = v;
  }
}
