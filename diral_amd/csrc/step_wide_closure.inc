// step_wide_closure.inc - the coded merge + finalize of step_wide_kernel<VPL, ..., PACKED> (dense topologies: BASELINE
// configs[2] at VPL = 4, configs[4] at VPL = 2); textual inclusion, like step_wide_pass.inc.  Leaves `passbits` behind.
// (The comments speak of VPL = 4: 256 viewers, 32 columns per wave, 8 K steps; VPL = 2 halves each.)
//
// Vehicle.received_update for every (resource, receiver), resources ascending (vehicle.py:35-47, test_env.py:204-240,
// SURVEY Q1-Q3) used to be a chain of 64 store -> gather -> OR steps PER PASS of 8 subject columns (4 passes per wave).
// Within a slot the transmitters of resource i never receive on i, so the table rows obey R_i = (I + E_i) R_{i-1} over
// (OR, AND), E_i holding at most one source per receiver: final = P . stamped with P = (I + E_A) ... (I + E_1), an N x N
// BIT matrix that depends on actions and positions only (profiles/micro/closure_merge.hip: cycle counts, bit equality).
//   1. closure (step_wide.hpp, beside P1): waves 6 and 7 walk the chain ONCE, on bits - wave 6 + c carries the source bits
//      [128 c, 128 c + 128) of every viewer's row of P, rows in LDS: gather the source's 16 bytes, ds_or them into the
//      own row (no register copy, no store, no VALU OR) - as the six P1 waves finish the rows of the gather table, and
//      leave P as bytes [viewer][lane group][K step] before the barrier that ends P1;
//   2. product, per pass of 16 subject columns: D[subject][viewer] = sum over sources A[subject][source] B[source][viewer]
//      on v_mfma_f32_16x16x32_bf16: a code (0xff << lag) & 0xff travels as the power of two 2^(16 popcount - 127) (bf16
//      bits: popcount << 11; the stamp of vehicle.py:56-70 folded in: popcount(raw & 0x7f), the own entry 8), P as
//      0.0 / 1.0.  A sum of at most 256 such terms has the exponent field 16 p ... 16 p + 8 of its largest term: the
//      merged code is (0xff00 >> (bits >> 27)) & 0xff - the (max, x) semiring read off the exponent of an ordinary f32
//      accumulation, exact whatever the rounding.  A operand: each lane loads the 8 consecutive source words of its
//      subject's quad row (2 x 16 B per K step of 32 sources; 32 VGPRs for the whole K range); B operand: the lane's byte
//      of P picks a 16-byte row of a 256-entry bits -> 8 x bf16 table in LDS.  The K index (source) is laid out
//      identically in A and B, so the product does not depend on the hardware's K order; the C/D layout
//      (cdna_hip_programming.md 3) puts four consecutive subjects of one viewer into the four accumulators of a lane =
//      one code word, and a 4 x 4 transpose of 16-lane rows (v_permlane32_swap, v_permlane16_swap) brings four
//      16-viewer tiles into the table's own lane = viewer arrangement.  (On 32 x 32 x 16 tiles a table row feeds twice
//      the multiply-adds, but the A operand of 32 columns takes 64 VGPRs: the kernel spilled 180 registers around it
//      and moved 7 GB per launch instead of 4 - HBM-bound at 2.0 ms.)
//   3. finalize per viewer slot (64 viewers x the pass's 16 columns): ages, stores, xpos by (subject, lag) from a
//      per-wave [column][lag] table filled from the ring rows, histogram.
// Flagged passes (a quad with an entry beyond the codes) are left to the loop behind this file, unchanged.
  unsigned int passbits = 0u;                      // bit pch: a quad of pass pch was flagged when the slot began
  {
    static_assert(WAVES == 8 && CPW == 8 * VPL && PC == 8 && NW == 2, "the closure merge is laid out for 8 waves x 16 / 32 columns x 128 / 256 viewers");
    constexpr int KS = NPAD / 32;                       // K steps of 32 sources
    constexpr int QW = CPW / 4;                         // quad rows of a wave
    typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
    typedef __attribute__((ext_vector_type(4))) float f32x4;
    typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
    typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
    const bool tables = !(EXTRA && RICH && p.notab);      // (uniform over the workgroup) no piggybacked tables: nothing to merge
    if (tables) {
      // P bytes and the bits -> bf16 table sit at compile-time LDS addresses right behind the merge scratch
      // (wide_lds_layout), so that the product's reads carry them as DS immediate offsets; the dynamic LDS segment starts
      // at address 0 when the kernel has no static LDS - checked, not assumed
      constexpr unsigned int kPb = kClPb, kLut = kClLut;
      if (!lds_base_is_zero) __builtin_trap();
      const int kbase = wave * CPW;
      const bool has_cols = kbase < NRows;                // (uniform) waves past the last subject row only help with the closure
      const int NQ = NRows >> 2;
      const size_t qrow0 = (size_t)b * NQ + (kbase >> 2);
      DIRAL_WCLOCK(tc0);
      unsigned int tkov = 0u;                            // lane c < 32: column c's fresh sequence number
      const int c16 = lane & 15, g4 = lane >> 4;         // product: lane = (subject or viewer of the tile, K group)
      unsigned char* const xt2 = reinterpret_cast<unsigned char*>(sw) + 64;   // [column][lag] -> xpos, 8 doubles per column
      // (the wave's columns - which passes are clean, fresh sequence numbers, the [column][lag] -> xpos table - and the A
      // operand of a pass: `cl_prologue` / `cl_build_a`, step_wide_body.inc)
      cl_stable = cl_far_guard();
      cl_prologue();
      passbits = cl_passbits;
      tkov = cl_tkov;
      ovf = ovf || cl_ovf;
      const global_ptr<unsigned int> tcrow = uniform_ptr(g_tcode, qrow0 * NV);
      const global_ptr<unsigned int> tarow = uniform_ptr(g_tage, qrow0 * NV);
      const unsigned int pbl = ((unsigned int)c16 * 4u + (unsigned int)g4) * (unsigned int)KS;   // this lane's KS bytes of a viewer's row of P
      const int jown = kbase >> 6;                         // the viewer slot that holds the own entries of this wave's columns
      const unsigned int oc = ul - (unsigned int)(kbase & 63);   // ... lane (kbase & 63) + c holds column c's
      unsigned int hand = 0u;                              // bit q: this lane handed an entry of quad q over (now 7 behind)
      // inv_w * 2^20 (exact: the exponent field + 20) and K * 2^20: the fixed-point bin
      const double inv_w20 = __hiloint2double(__double2hiint(inv_w) + (20 << 20), __double2loint(inv_w));
      const unsigned int k20 = (unsigned int)K << 20;
      const int nqv = FULL ? QW : ((NRows - kbase) >> 2 < QW ? (NRows - kbase) >> 2 : QW);   // quad rows of this wave that exist
#pragma unroll 1
      for (int pass = 0; pass < CPW / 16; ++pass) {
        DIRAL_WCLOCK(tc0);
        // A operand: [K step of 32 sources] 8 x bf16 of this lane's subject (cl_a)
        const bool pass_cols = has_cols && (FULL || kbase + 16 * pass < NRows);
        if (pass_cols) cl_build_a(pass);
        DIRAL_WCLOCK(tc1);
#ifdef DIRAL_TIMING
        acc_load += tc1 - tc0;
#endif
        if (!pass_cols) continue;
#pragma unroll 1
        for (int j = 0; j < VPL; ++j) {
          DIRAL_WCLOCK(tc2);
          // the raw code / age words of this slot's four quads, requested in front of the product (which covers their round
          // trip; a load inside the quad loop was a round trip to L2 per quad, and its s_waitcnt vmcnt also waited for the
          // stores of the quad before).  Quads that do not exist: the last one that does.
          unsigned int rawv[4], agv[4];
#pragma unroll
          for (int qq = 0; qq < 4; ++qq) {
            const int qx = 4 * pass + qq;
            const unsigned int o = (unsigned int)((qx < nqv ? qx : nqv - 1) * NV) + ul + 64u * (unsigned int)j;
            rawv[qq] = tcrow[o];                               // (the A operand's loads brought the line to L2 a moment ago)
            agv[qq] = __builtin_nontemporal_load(&tarow[o]);   // (read once and written once per slot)
          }
          // ---- 2. product: the merged code words of viewer slot j (64 viewers = four 16-viewer tiles) x 16 columns
          unsigned int kpn[4];
          {
            unsigned int res[4];
            // (the four tiles with four accumulators taking the K steps round-robin instead of a tile at a time: measured
            // no faster - the table rows, not the dependent MFMAs, pace this loop)
#pragma unroll
            for (int tt = 0; tt < 4; ++tt) {
              // this lane's viewer of the tile: 64 j + 16 tt + c16; its table indices (one byte per K step) in one read
              f32x4 acc = {0.f, 0.f, 0.f, 0.f};
              const unsigned int pba = kPb + pbl + ((64u * (unsigned int)j + 16u * (unsigned int)tt) * (4u * (unsigned int)KS));
              unsigned int idx0, idx1 = 0u;
              if constexpr (KS == 8) {
                const u32x2 idx = *lds_at<u32x2>(pba);
                idx0 = idx.x; idx1 = idx.y;
              } else {
                idx0 = *lds_at<unsigned int>(pba);
              }
              // the B operand of K step n: the table row(s) of byte n of the index word
              auto brow = [&](auto ntag, unsigned int w) -> u32x4 {
                return *lds_at<u32x4>(kLut + lut_row<decltype(ntag)::value>(w));
              };
              {
                const u32x4 b0 = brow(std::integral_constant<int, 0>{}, idx0);
                const u32x4 b1 = brow(std::integral_constant<int, 1>{}, idx0);
                const u32x4 b2 = brow(std::integral_constant<int, 2>{}, idx0);
                const u32x4 b3 = brow(std::integral_constant<int, 3>{}, idx0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cl_a[0]), __builtin_bit_cast(bf16x8, b0), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cl_a[1]), __builtin_bit_cast(bf16x8, b1), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cl_a[2]), __builtin_bit_cast(bf16x8, b2), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cl_a[3]), __builtin_bit_cast(bf16x8, b3), acc, 0, 0, 0);
              }
              if constexpr (KS == 8) {
                const u32x4 b4 = brow(std::integral_constant<int, 0>{}, idx1);
                const u32x4 b5 = brow(std::integral_constant<int, 1>{}, idx1);
                const u32x4 b6 = brow(std::integral_constant<int, 2>{}, idx1);
                const u32x4 b7 = brow(std::integral_constant<int, 3>{}, idx1);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cl_a[KS - 4]), __builtin_bit_cast(bf16x8, b4), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cl_a[KS - 3]), __builtin_bit_cast(bf16x8, b5), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cl_a[KS - 2]), __builtin_bit_cast(bf16x8, b6), acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cl_a[KS - 1]), __builtin_bit_cast(bf16x8, b7), acc, 0, 0, 0);
              }
              // accumulator r = subject 16 pass + 4 g4 + r of the wave, viewer 64 j + 16 tt + c16: the bytes of one code word
              unsigned int word = 0u;
#pragma unroll
              for (int r = 0; r < 4; ++r) word |= ((0xff00u >> (__float_as_uint(acc[r]) >> 27)) & 0xffu) << (8 * r);
              res[tt] = word;
            }
            // tile tt, 16-lane row g holds (quad g, viewers 16 tt + c); wanted: word q, row tt = (quad q, viewers 16 tt + c)
            const auto s02 = __builtin_amdgcn_permlane32_swap(res[0], res[2], false, false);
            const auto s13 = __builtin_amdgcn_permlane32_swap(res[1], res[3], false, false);
            const auto n01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
            const auto n23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
            kpn[0] = n01[0]; kpn[1] = n01[1]; kpn[2] = n23[0]; kpn[3] = n23[1];
          }
          DIRAL_WCLOCK(tc3);
#ifdef DIRAL_TIMING
          acc_merge += tc3 - tc2;
#endif
          // ---- 3. ages, stores, xpos, histogram of this viewer slot
          const bool uval = FULL || (lane + 64 * j < N);
          const unsigned int uo = ul + 64u * (unsigned int)j;
          const double npx_j = s_npx[uo];                                      // this viewer's post-move position
          const double cfix_j = (pRb - npx_j) * inv_w20;
          unsigned int* const hrow_j = s_hist + uo * (unsigned int)KP;         // ... and its histogram row (two 16-bit bins per word)
          // (rolled over the pass's four quads, the merged words rotating through element 0: a dynamically indexed register
          // array would live in scratch memory)
#pragma unroll 1
          for (int qq = 0; qq < 4; ++qq) {
            const int q = 4 * pass + qq;                                     // quad of the wave's eight
            const unsigned int kq = kpn[0], raw = rawv[0], ag = agv[0];
#pragma unroll
            for (int i = 0; i < 3; ++i) { kpn[i] = kpn[i + 1]; rawv[i] = rawv[i + 1]; agv[i] = agv[i + 1]; }
            if ((passbits >> (q >> 1)) & 1u) continue;                       // (uniform) a flagged pass: the loop below
            if (!FULL && kbase + 4 * q >= NRows) continue;                   // (uniform) no such subject rows
            // Vehicle.periodic_update (vehicle.py:56-70): every lag + 1 (a shift), every age + 1 (saturating, packed), the
            // own entry: lag 0 / age 0.  Padded viewer slots (u >= N) read whatever lies behind the row: masked to 0.
            const unsigned int ocq = oc - 4u * (unsigned int)q;
            const unsigned int ob = (j == jown && ocq < 4u && (FULL || kbase + (int)oc < N)) ? 0xffu << (8u * ocq) : 0u;
            const unsigned int c0 = uval ? raw : 0u, a0 = uval ? ag : 0u;
            const unsigned int kp0 = ((c0 << 1) & 0xfefefefeu) | ob;
            const unsigned int hi = a0 & 0x80808080u, lo = (a0 & 0x7f7f7f7fu) + 0x01010101u, sat = lo & hi;
            unsigned int agq = ((lo ^ hi) | sat | (sat - (sat >> 7))) & ~ob;
            const unsigned int kn = uval ? kq : 0u;
            unsigned int kmask = 0u;                                           // (uniform) bytes of subjects k >= N: never counted
            if constexpr (!FULL) {
#pragma unroll
              for (int cc = 0; cc < 4; ++cc) kmask |= (kbase + 4 * q + cc < N) ? 0u : 0xffu << (8 * cc);
            }
            {
              // ages of updated entries cleared with a byte mask of the code bytes that changed; the two words go back
              const unsigned int x = kn ^ kp0;
              const unsigned int nz = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
              agq &= ~(nz | (nz - (nz >> 7)));
            }
            if (uval) {
              __builtin_nontemporal_store(kn, &tcrow[(unsigned int)(q * NV) + uo]);
              __builtin_nontemporal_store(agq, &tarow[(unsigned int)(q * NV) + uo]);
            }
            // One entry per lane and column (the body of step_fast64's fast quad, csrc/step_fast64.hpp P3b): whether the
            // entry counts - vehicle and subject exist, not the own entry, age < limit (network.py:547) - is ONE byte compare
            // against the age word with those bytes forced to 255; the bin in fixed point: ti = trunc((v + Rb) * inv_w * 2^20),
            // 0 <= ti <= K * 2^20 is the range test |v| < Rb, ti >> 20 the bin, and when the 20 fraction bits are neither
            // all 0 nor all 1 the value is at least 2^-20 bin widths inside that bin (hist_bin_estimate: the estimate is
            // within 2^-45 of exact) - else (an edge hit, |v| at Rb) the lane takes the exact NumPy statement, behind a
            // uniform branch.  Three of four entries of a 4 km highway lie beyond the bin range: the histogram increment
            // stays predicated.
#ifndef DIRAL_WIDE_KSLOTS
            const unsigned int agt = (uval ? (agq | ob) : 0xffffffffu) | kmask;
#else /* DIRAL_WIDE_KSLOTS */
            // (K slots without the histogram: every byte "past the age limit" - nothing counts, no plane xpos is fetched for
            // counting; the hand-overs to the planes still happen)
            const unsigned int agt = tally_on ? ((uval ? (agq | ob) : 0xffffffffu) | kmask) : 0xffffffffu;
#endif /* DIRAL_WIDE_KSLOTS */
            // Network.dist_piggy + get_positional_dist_2_piggy (network.py:538-558, 473-513) of the entry at xpos xg; all
            // y == 0: v = x1 - x2 IS d * sign exactly, d = |v| (see step_fast64.hpp)
            auto exact_bin = [&](double xg, bool& cnt) -> int {               // (rare: an exact edge hit, |v| at Rb)
              double vv = xg - npx_j;
              cnt = __builtin_fabs(vv) < pRb;
              int bin = 0;
              if (cnt) {
                bool unsafe;
                bin = hist_bin_clamp(hist_bin_estimate(vv, pRb, inv_w, K, unsafe), K);
                if (((unsigned int)__double2hiint(vv) & 0x7fffffffu) < 0x20b00000u) {   // |v| below 2^-500 (its square underflows) or 0
                  const double d = dist_general(npx_j - xg, 0.0);
                  vv = (vv > 0.0) ? d : -d;
                }
                const double e0 = s_edges[bin], e1 = s_edges[bin + 1];
                bin += (vv >= e1 ? 1 : 0) - (vv < e0 ? 1 : 0);
              }
              return bin;
            };
            // a byte with (code & 0x7f) == 0 in some lane: a never-heard entry or a hand-over - the quad goes column by column
            const bool rare = uval && (((kn & 0x7f7f7f7fu) + 0x7f7f7f7fu) & 0x80808080u) != 0x80808080u;
            // ... which needs the column loop only for a hand-over (code 0x80) or an entry without a code that can still COUNT
            // (age below the limit, network.py:547: its xpos lives in the plane).  On a highway that broke apart half the
            // viewers of a column hold entries beyond the codes, nearly all of them long past the age limit: those take the
            // common path - their lookup reads the pad below the column's row, their age keeps them out of the histogram.
            // (the finer test runs only behind the coarse one: clean envs never pay for it)
            // (N <= 128 only: at N > 128 the packed form runs on dense topologies without such entries, and the extra code in the
            // loop measured + 1 % on C3)
            bool slowq = VPL == 4 && rare;
            if (VPL == 2 && __ballot(rare) != 0ull) {
              const unsigned int z = ~((kn & 0x7f7f7f7fu) + 0x7f7f7f7fu) & 0x80808080u;     // bytes whose low seven bits are 0
              unsigned int y = 0x80808080u;                                                // bytes with age < limit (limits above 127: all)
              if (age_limit <= 127) y = ~((((agt & 0x7f7f7f7fu) | 0x80808080u) - 0x01010101u * (unsigned int)age_limit) | agt) & 0x80808080u;
              slowq = uval && (z & ((kn & 0x80808080u) | y)) != 0u;
            }
            double xs[4];
            if (__ballot(slowq) != 0ull) {
#pragma unroll
              for (int cc = 0; cc < 4; ++cc) {
                const unsigned int rf = (kn >> (8 * cc)) & 255u;
                // the lag is the count of trailing zeros of the code byte (-1: never heard - the row below, overwritten)
                const int lag = ffbl_byte<0>(rf);
                double xg = *reinterpret_cast<const double*>(xt2 + q * 256 + cc * 64 + lag * 8);
                if ((rf & 0x7fu) == 0u) {                                      // 0: never heard; 0x80: lag 7
                  const int k = kbase + 4 * q + cc;
                  const global_ptr<double> txrow = uniform_ptr(p.tx, (bR + k) * NV);
                  if (rf == 0u) {                                              // never heard, or beyond the codes: the xpos lives in the plane
                    // (wanted only where the entry can count - network.py:547 -: on a highway that broke apart half the viewers
                    // of a column hold entries this old, nearly all of them past the age limit; the load is a round trip to HBM per
                    // column, skipped as a whole when no lane needs it)
                    if (((agt >> (8 * cc)) & 255u) < (unsigned int)age_limit) {
                      xg = txrow[uo];
                      asm volatile("" : "+v"(xg));                              // (consumed inside the branch: see step_fast64.hpp)
                    }
                  } else if (FULL || (uval && k < N)) {
                    // from the next slot on beyond the codes: hand over - sequence number (lag 7) and xpos go to the planes
                    const global_ptr<unsigned int> tkrow = uniform_ptr(p.tkey, (bR + k) * NV);
                    const unsigned int tk_own = (unsigned int)__builtin_amdgcn_readlane((int)tkov, 4 * q + cc);
                    tkrow[uo] = ((tk_own - 7u) << 8) | ((agq >> (8 * cc)) & 255u);
                    txrow[uo] = xg;
                    hand |= 1u << q;
                  }
                }
                xs[cc] = xg;
              }
            } else {
              // the common quad: the four xpos lookups in flight together (a column at a time, each lookup waited for before
              // the next was issued, cost a wave four LDS round trips and a dozen exec-mask branches per quad)
              xs[0] = *reinterpret_cast<const double*>(xt2 + q * 256 + 0 * 64 + ffbl_byte<0>(kn) * 8);
              xs[1] = *reinterpret_cast<const double*>(xt2 + q * 256 + 1 * 64 + ffbl_byte<1>(kn) * 8);
              xs[2] = *reinterpret_cast<const double*>(xt2 + q * 256 + 2 * 64 + ffbl_byte<2>(kn) * 8);
              xs[3] = *reinterpret_cast<const double*>(xt2 + q * 256 + 3 * 64 + ffbl_byte<3>(kn) * 8);
            }
            // the four bins side by side, ONE test for the rare exact-edge statement
            // ti = trunc(((xpos - npx) + Rb) * inv_w * 2^20) as ONE fused multiply-add, xpos * (inv_w 2^20) + cfix_j with
            // cfix_j = (Rb - npx) * inv_w 2^20 once per viewer slot: ti only has to be within 2^-20 bin widths of the exact
            // quotient (an estimate nearer an edge than that takes the exact NumPy statement below, as before), and either
            // form is within 2^-45.  The histogram word and increment come straight from ti: bin = ti >> 20, word = bin >> 1,
            // half = bin & 1 (the exact statement hands back bin << 20).
            int tiv[4];
            bool cntv[4], needv[4];
            bool anyneed = false;
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
              const int ti = cvt_i32_f64_sat(__builtin_fma(xs[cc], inv_w20, cfix_j));
              const bool agev = ((agt >> (8 * cc)) & 255u) < (unsigned int)age_limit;
              const bool m = agev && (unsigned int)ti <= k20;
              needv[cc] = m && ((unsigned int)(ti + 1) & 0xfffffu) <= 1u;
              cntv[cc] = m;                                                // (an edge hit: decided below)
              anyneed = anyneed || needv[cc];
              tiv[cc] = ti;
            }
            if (__ballot(anyneed) != 0ull) {
#pragma unroll
              for (int cc = 0; cc < 4; ++cc)
                if (needv[cc]) tiv[cc] = exact_bin(xs[cc], cntv[cc]) << 20;
            }
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
              if (cntv[cc]) {
                const unsigned int t = (unsigned int)tiv[cc];
                atomicAdd(reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned char*>(hrow_j) + ((t >> 21) << 2)),
                          ((t >> 20) & 1u) * 0xffffu + 1u);
              }
            }
          }
#ifdef DIRAL_TIMING
          DIRAL_WCLOCK(tc2);
          acc_fin += tc2 - tc3;
#endif
        }
      }
      if (has_cols) {
#pragma unroll
        for (int q = 0; q < QW; ++q) {
          if (__ballot((hand >> q) & 1u) != 0ull && lane == 0) { g_told[qrow0 + q] = 1u; s_slow[0] = 1u; }
        }
      }
    }
  }
