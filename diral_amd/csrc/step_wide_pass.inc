// step_wide_pass.inc - one pass over PC subject columns of the (seq, age) plane `tkey` (round-2 form): load + stamp, merge
// (thermometer codes, byte ranks, or 32-bit keys), finalize.  Included TWICE by step_wide_body.inc - the pass of the plane-form
// handles, and the flagged pass of the packed form - with DIRAL_PASS_THERMO_FIRST set by the includer; textual inclusion, because
// a lambda called from the two loops trips a backend error ("illegal VGPR to SGPR copy") in this compiler.
// In steady state the lag of an entry behind its subject's own sequence number is tiny (C3: <= 4, C2: <= 5, C5: <= 7 for 98 %
// of the entries - profiles/lag_distribution.py), so a pass first tries thermometer codes (thermo_codes(), wave_ops.hpp): ONE
// v_or_b32 merges the four columns of a word where the byte ranks take four SDWA maxes.  Exact while every entry of the pass
// has lag <= 7 or was never heard; otherwise the pass is redone with byte ranks (lag < 255), then with 32-bit keys.
// Expects `kbase` in scope; leaves `tkov` (lane c: column c's fresh sequence number) behind.
    // One packed pass, ONE body for both packed representations (two copies of it cost 12 more spilled
    // registers): the table words are loaded and turned into clamped lag bytes - 0..7 and 12 = never heard for the
    // thermometer codes, 0..253 and 255 for the byte ranks - and if an entry does not fit the codes the loads are
    // simply repeated with the other pair of constants.  Only the merge loop exists per representation.
    bool thermo = DIRAL_PASS_THERMO_FIRST;
    bool packed_ok;
    unsigned int kp[NK], agew[NK];               // [word * VPL + slot]: 4 lag bytes (then codes / ranks) each; ages, same packing
    unsigned int tkov;                           // lane c: column c's fresh sequence number of its subject
    // byte ranks: entries 254 and more stamps behind share the lowest rank (1) as long as they all hold ONE sequence
    // number per column - lane c keeps it: an env whose highway broke into clusters that no longer hear each other
    // carries such entries for ever (every viewer of a cluster converges on the last stamp that crossed), and the 32-bit
    // path - a 64-step chain per COLUMN - is kept for columns with two different ones (imported tables, the transient)
    // (N <= 128 only: at N > 128 the two registers it keeps across the pass cost the packed form's coded loop 13 spilled
    // VGPRs - C3 + 2 % -, and the dense topologies that run packed there never break apart)
    constexpr bool FARRANK = VPL == 2;
    unsigned int farseq = 0u;
    bool farbad = false;
#if DIRAL_PASS_PACKED_IO
    // (the flagged pass of the packed form, reading and writing the packed words itself)
    unsigned int cwp[NK], awp[NK];               // the pass's code and age words as the slot found them
    {
      const unsigned int cl = ul < (unsigned int)PC ? ul : 0u;
      const bool cv = ul < (unsigned int)PC && (FULL || kbase + (int)cl < N);
      tkov = cv ? tsrow[cl] + 1u : 0u;            // the subjects' own sequence numbers (`tseq`), stamped: + 1 (vehicle.py:62)
      ovf = ovf || (cv && tkov >= (1u << 24) - 1u);
#pragma unroll
      for (int w = 0; w < NW; ++w)
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          cwp[w * VPL + j] = tcrow[(unsigned int)(w * NV) + ul + 64u * j];
          awp[w * VPL + j] = tarow[(unsigned int)(w * NV) + ul + 64u * j];
        }
    }
#else
    {
      // the subjects' own sequence numbers: lane c reads the diagonal entry of column c (one load for the pass instead of
      // a v_readlane + select per column and slot); stamped: + 1 (vehicle.py:62)
      const global_ptr<const unsigned int> row0 = uniform_ptr<const unsigned int>(p.tkey, (bR + kbase) * NV);
      const unsigned int cl = ul < (unsigned int)PC ? ul : 0u;
      const bool cv = ul < (unsigned int)PC && (FULL || kbase + (int)cl < N);
      const unsigned int wd = row0[cl * (unsigned int)(NV + 1) + (unsigned int)kbase];
      tkov = cv ? (wd >> 8) + 1u : 0u;
      ovf = ovf || (cv && tkov >= (1u << 24) - 1u);
    }
#endif
    // the own entries of the pass: lane (kbase & 63) + c of viewer slot kbase >> 6 holds column c's (PC columns never
    // straddle a 64-viewer slot); patched in the packed words: lag 0, age 0
    unsigned int ownm[NW];
    {
      const unsigned int oc = ul - (unsigned int)(kbase & 63);
      const unsigned int om = oc < (unsigned int)PC ? 0xffu << (8u * (oc & 3u)) : 0u;
#pragma unroll
      for (int w = 0; w < NW; ++w) ownm[w] = (oc >> 2) == (unsigned int)w ? om : 0u;
    }
    for (;;) {
    // lag byte of an entry the subject's owner is `lag` stamps ahead of: min(lag, cap); never heard (seq 0): `nh`.
    // A byte in (limit, cap] does not fit the representation (codes: lag 8 and more; ranks: 254 and more)
    const unsigned int lag_cap = thermo ? 11u : 254u, lag_nh = thermo ? 12u : 255u;
    DIRAL_WCLOCK(tc0);
    // -- load + Vehicle.periodic_update (vehicle.py:56-70), lags behind the subject's
    //    own fresh sequence number
#pragma unroll
    for (int q = 0; q < NK; ++q) { kp[q] = 0u; agew[q] = 0u; }
    farbad = false;
    // (16 table words in flight at a time: LC columns x VPL slots)
    constexpr int LC = DIRAL_WIDE_INFLIGHT / VPL;
#pragma unroll
    for (int c0 = 0; c0 < PC; c0 += LC) {
    unsigned int wraw[LC * VPL];
#pragma unroll
    for (int c = 0; c < LC; ++c) {
      const global_ptr<const unsigned int> row = uniform_ptr<const unsigned int>(p.tkey, (bR + kbase + c0 + c) * NV);   // rows are padded to 16: in bounds
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
#if DIRAL_PASS_PACKED_IO
        // `tkey` answers for code-0 entries only (never heard, or beyond the codes); the others come from the code words
        const unsigned int rc = (cwp[((c0 + c) >> 2) * VPL + j] >> (8 * ((c0 + c) & 3))) & 255u;
        wraw[c * VPL + j] = rc == 0u ? row[ul + 64u * j] : 0u;
#else
        wraw[c * VPL + j] = row[ul + 64u * j];
#endif
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int c = c0; c < c0 + LC; ++c) {
      const int k = kbase + c;
      const bool kval = FULL || k < N;
      const unsigned int t = (unsigned int)__builtin_amdgcn_readlane((int)tkov, c);
      bool farj[VPL];
      unsigned long long farm = 0ull;
#pragma unroll
      for (int j = 0; j < VPL; ++j) {
        const int u = lane + 64 * j;
#if DIRAL_PASS_PACKED_IO
        // the entry as a (seq, age) word, unstamped: a coded one from the subject's own number and the lag
        unsigned int w;
        {
          const unsigned int rc = (cwp[(c >> 2) * VPL + j] >> (8 * (c & 3))) & 255u, ac = (awp[(c >> 2) * VPL + j] >> (8 * (c & 3))) & 255u;
          const unsigned int sq = rc ? t - 9u + (unsigned int)__popc(rc) : (wraw[(c - c0) * VPL + j] >> 8);
          w = (FULL || (kval && u < N)) ? ((sq << 8) | ac) : 0u;
        }
#else
        const unsigned int w = (FULL || (kval && u < N)) ? wraw[(c - c0) * VPL + j] : 0u;
#endif
        const unsigned int age = min((w & 255u) + 1u, 255u);
        const unsigned int lag = min(t - (w >> 8), lag_cap);
        const unsigned int lagc = w < 256u ? lag_nh : lag;
        kp[(c >> 2) * VPL + j] |= lagc << (8 * (c & 3));
        agew[(c >> 2) * VPL + j] |= age << (8 * (c & 3));
        farj[j] = FARRANK && !thermo && w >= 256u && lag >= 254u;
        if constexpr (FARRANK) farm |= __ballot(farj[j]);
      }
      if (FARRANK && farm != 0ull) {               // (uniform, rare) far entries: one sequence number for the column?
        unsigned int ref = 0u;
        bool have = false;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          const unsigned long long m = __ballot(farj[j]);
          const unsigned int w = wraw[(c - c0) * VPL + j];
          if (!have && m != 0ull) { ref = (unsigned int)__builtin_amdgcn_readlane((int)(w >> 8), __builtin_ctzll(m)); have = true; }
        }
#pragma unroll
        for (int j = 0; j < VPL; ++j) farbad = farbad || (farj[j] && (wraw[(c - c0) * VPL + j] >> 8) != ref);
        farseq = ul == (unsigned int)c ? ref : farseq;
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    }
    // the own entries: lag 0 / age 0 (vehicle.py:61-64)
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
      if (j == (kbase >> 6)) {                     // wave-uniform
#pragma unroll
        for (int w = 0; w < NW; ++w) { kp[w * VPL + j] &= ~ownm[w]; agew[w * VPL + j] &= ~ownm[w]; }
      }
    }
    // does every byte fit?  Codes: a byte in 8..11 (bit 3 without bit 2) does not; ranks: 254 does not
    unsigned int badw = 0u;
    if (thermo) {
#pragma unroll
      for (int q = 0; q < NK; ++q) badw |= (kp[q] >> 3) & ~(kp[q] >> 2);
      badw &= 0x01010101u;
    } else {
      if constexpr (FARRANK) {
        badw = farbad ? 1u : 0u;                   // (a byte of 254: fine while its column holds one far sequence number)
      } else {
#pragma unroll
        for (int q = 0; q < NK; ++q) { const unsigned int y = kp[q] ^ 0xfefefefeu; badw |= (y - 0x01010101u) & ~y; }
        badw &= 0x80808080u;
      }
    }
    packed_ok = (__ballot(badw != 0u) == 0ull);
    DIRAL_WCLOCK(tc1);
    if (packed_ok || !thermo) break;
    thermo = false;
    }
    if (packed_ok) {
      // lag bytes -> thermometer codes, or byte ranks 255 - lag (the complement; 255 -> 0: never heard)
#pragma unroll
      for (int q = 0; q < NK; ++q) kp[q] = thermo ? thermo_codes(kp[q]) : ~kp[q];
      const unsigned int seq_base = thermo ? 8u : 255u;
      unsigned int kp0[NK];                      // the ranks before the merge
#pragma unroll
      for (int q = 0; q < NK; ++q) kp0[q] = kp[q];
      // -- Vehicle.received_update for every (resource, rx), resources ascending:
      //    rank[u] = max(rank[u], rank[m_i(u)]), 4 columns per word, byte-wise (SDWA)
      {
      // vector layout sv[viewer] = its NW words: ONE 8/16-byte gather per slot and step.  A step is a
      // dependent chain (gather -> max -> write-back -> next gather, in-order LDS queue), so the
      // wider pass halves the number of chains a wave walks per column.
      typedef unsigned int uvec __attribute__((ext_vector_type(NW)));
      uvec* const sv = reinterpret_cast<uvec*>(sw);
      auto put_slot = [&](int j) {
        uvec t;
#pragma unroll
        for (int w = 0; w < NW; ++w) t[w] = kp[w * VPL + j];
        sv[lane + 64 * j] = t;
      };
#pragma unroll
      for (int j = 0; j < VPL; ++j) put_slot(j);
      wave_lds_order();
      auto merge_loop = [&](auto wtag, auto ttag) {
        constexpr int W = decltype(wtag)::value;
        constexpr bool THERMO = decltype(ttag)::value;
        const unsigned char* const swb = reinterpret_cast<const unsigned char*>(sw);
        unsigned long long rem = actw;
        unsigned int m_next = rem ? (unsigned int)s_mtab[__builtin_ctzll(rem) * MT + lane] : 0u;
        while (rem) {
          const unsigned long long low = rem & (0ull - rem);     // this step's resource, as its bit
          rem ^= low;
          const unsigned int mw = m_next;
          if (rem) m_next = (unsigned int)s_mtab[__builtin_ctzll(rem) * MT + lane];
          // the words of this step's transmitters, as the earlier steps left them (a receiver that is no transmitter
          // of i reads its OWN possibly stale words where it has no source: a subset of what it holds, a no-op)
#pragma unroll
          for (int j = 0; j < VPL; ++j) {
            if (VPL == 2 || (txs[j] & low)) put_slot(j);    // (N <= 128, two slots: the tests cost more than the stores they save)
          }
          wave_lds_order();
          unsigned int v[NK], sa[VPL];
          unpack_src<VPL, (NW == 2 ? 3u : 4u)>(mw, sa);
#pragma unroll
          for (int j = 0; j < VPL; ++j) {
            const uvec g = W >= 0 ? *lds_at<uvec>(SCR * (W >= 0 ? W : 0) + sa[j]) : *reinterpret_cast<const uvec*>(swb + sa[j]);
#pragma unroll
            for (int w = 0; w < NW; ++w) v[w * VPL + j] = g[w];
          }
          wave_lds_order();
          if constexpr (THERMO) {
#pragma unroll
            for (int q = 0; q < NK; ++q) kp[q] |= v[q];
          } else {
            max_u8_words<NK>(kp, v);
          }
        }
      };
      auto merge_codes = [&](auto wtag) { merge_loop(wtag, std::true_type{}); };
      auto merge_ranks = [&](auto wtag) { merge_loop(wtag, std::false_type{}); };
      if (thermo) DIRAL_WIDE_DISPATCH_WAVE(merge_codes);
      else DIRAL_WIDE_DISPATCH_WAVE(merge_ranks);
      }
      DIRAL_WCLOCK(tc2);

      // -- xpos by (subject, sequence number); histogram.  One column at a time (rolled: uniform byte
      //    extraction).  The rank -> xpos table of the column: the subject's 8 latest stamps from its ring row
      //    (lane l < 8 * PC holds lag l & 7 of column l >> 3, loaded once per pass), the few older entries
      //    scatter their xpos from the plane; then EVERY entry reads its xpos by its final rank.
      // (the two representations differ in constants only - wave-uniform scalars, not per-entry selects:)
      const unsigned int old_thr = thermo ? 0u : 247u;                  // rank <= old_thr: older than the ring reaches (codes: never heard)
      const unsigned int at7_val = thermo ? 0x80u : 248u;                // the rank / code of lag 7
      const unsigned int far_sub = thermo ? 0x80u : 1u, far_thr = thermo ? 0u : 247u;   // heard and lag >= 7: rank - far_sub <= far_thr
      const unsigned int xt_l = thermo ? ((0xffu << (ul & 7u)) & 0xffu) : 255u - (ul & 7u);   // the table slot of ring lag `lane & 7`
#if DIRAL_PASS_PACKED_IO
      unsigned int ncw[NK], naw[NK];             // the pass's code and age words as it leaves them
      bool keepw[NW];                            // word w holds an entry 7 or more behind: its quad stays flagged
#pragma unroll
      for (int q = 0; q < NK; ++q) { ncw[q] = 0u; naw[q] = 0u; }
#pragma unroll
      for (int w = 0; w < NW; ++w) keepw[w] = false;
#endif
      double rg = 0.0;
      {
        const unsigned int rc = ul >> 3, rl = ul & 7u;
        const unsigned int tkc = (unsigned int)__builtin_amdgcn_ds_bpermute((int)(rc << 2), (int)tkov);
        if (rc < (unsigned int)PC) rg = ringp[(size_t)(bR + kbase + rc) * 8 + ((tkc - rl) & 7u)];
      }
#pragma unroll
      for (int w = 0; w < NW; ++w)
#pragma unroll FIN_UNROLL
      for (int cc = 0; cc < 4; ++cc) {
        const int c = 4 * w + cc;
        const int k = kbase + c;
        const bool kvalid = FULL || k < N;
        const global_ptr<unsigned int> tkrow = uniform_ptr(p.tkey, (bR + k) * NV);
        const global_ptr<double> txrow = uniform_ptr(p.tx, (bR + k) * NV);
        const unsigned int tk_own = (unsigned int)__builtin_amdgcn_readlane((int)tkov, c);
        const unsigned int far_own = FARRANK ? (unsigned int)__builtin_amdgcn_readlane((int)farseq, c) : 0u;   // (ranks) the column's far sequence number
        const double pxk = s_px[kvalid ? k : 0];
        if ((ul >> 3) == (unsigned int)c) {
          // lag 0 is this slot's stamp (vehicle.py:61-63: the pre-move position under the fresh number)
          const unsigned int l = ul & 7u;
          xt[xt_l] = (l == 0u) ? pxk : rg;
          if (l == 0u && kvalid) ringp[(size_t)(bR + k) * 8 + (tk_own & 7u)] = pxk;
        }
        unsigned int rank0[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          const int u = lane + 64 * j;
          rank0[j] = pick(kp0, j, w, cc);
          // older than the ring reaches (codes: only the never-heard entries): the plane holds its xpos
          const bool old = rank0[j] <= old_thr;
          if (old && (FULL || (u < N && kvalid))) xt[rank0[j]] = txrow[ul + 64u * j];
        }
        wave_lds_order();
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          const unsigned int rf = pick(kp, j, w, cc);
          const double xg = xt[rf];
          const bool upd = rf != rank0[j];
          // sequence number back from the rank / from the code (lag = 8 - popcount)
          unsigned int seqf = rf ? tk_own - seq_base + (thermo ? (unsigned int)__popc(rf) : rf) : 0u;
          if (FARRANK && !thermo && rf == 1u) seqf = far_own;
          const unsigned int wn = (seqf << 8) | (upd ? 0u : pick(agew, j, w, cc));
          // the plane must hold the xpos of every entry the ring may not reach next slot: an entry that is now 7
          // behind, or a fresh copy of an older one
          const bool at7 = rf == at7_val;
          const bool far = rf - far_sub <= far_thr;
#if DIRAL_PASS_PACKED_IO
          {
            // the packed words of the next slot; `tkey` keeps the sequence number of an entry 7 or more behind (its code
            // byte is 0x80 now and 0 from the next stamp on)
            const bool lvf = FULL || ((lane + 64 * j < N) && kvalid);
            const unsigned int lagf = thermo ? 8u - (unsigned int)__popc(rf) : 255u - rf;
            const unsigned int codef = (rf != 0u && lagf <= 7u) ? ((0xffu << lagf) & 0xffu) : 0u;
            if (lvf) {
              ncw[w * VPL + j] |= codef << (8 * cc);
              naw[w * VPL + j] |= (wn & 255u) << (8 * cc);
              keepw[w] = keepw[w] || (seqf != 0u && lagf >= 7u);
              if (seqf != 0u && lagf >= 7u) tkrow[ul + 64u * j] = wn;
            }
          }
          emit(k, kvalid, j, far && (upd || at7), wn, xg, tkrow, txrow, std::integral_constant<int, 4>{});
#else
          emit(k, kvalid, j, far && (upd || at7), wn, xg, tkrow, txrow, std::integral_constant<int, 1>{});
#endif
        }
        wave_lds_order();
      }
#if DIRAL_PASS_PACKED_IO
      // the packed words, the fresh sequence numbers, the flags of the next slot
      if (ul < (unsigned int)PC) tsrow[ul] = tkov;
#pragma unroll
      for (int w = 0; w < NW; ++w) {
        const bool anyk = __ballot(keepw[w]) != 0ull;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          if (FULL || lane + 64 * j < N) {
            tcrow[(unsigned int)(w * NV) + ul + 64u * j] = ncw[w * VPL + j];
            tarow[(unsigned int)(w * NV) + ul + 64u * j] = naw[w * VPL + j];
          }
        }
        if (lane == 0) g_told[qrow + w] = anyk ? 1u : 0u;
        if (anyk && lane == 0) s_slow[0] = 1u;
      }
#endif
    } else {
      // -- 32-bit path, column by column: key = (seq << 8) | source viewer (imported or
      //    very stale tables: an entry with lag >= 255 and seq != 0)
#if DIRAL_PASS_PACKED_IO
      unpack_pass();                             // (this path walks `tkey`: the pass's entries as (seq, age) words first)
#endif
      DIRAL_WCLOCK(tc2);
      double* const sx = xt;
#pragma unroll 1
      for (int c = 0; c < PC; ++c) {
        const int k = kbase + c;
        const bool kvalid = k < N;
        const global_ptr<unsigned int> tkrow = uniform_ptr(p.tkey, (bR + k) * NV);
        const global_ptr<double> txrow = uniform_ptr(p.tx, (bR + k) * NV);
        unsigned int ws[VPL], key[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          const int u = lane + 64 * j;
          const bool lv = (u < N);
          unsigned int w = tkrow[lv ? u : 0];
          w = (lv && kvalid) ? w : 0u;
          const bool own = lv && (u == k);
          const unsigned int seq = (w >> 8) + (own ? 1u : 0u);
          const unsigned int a0 = w & 255u;
          ws[j] = (seq << 8) | (own ? 0u : (a0 + (a0 < 255u ? 1u : 0u)));
          key[j] = (ws[j] & ~255u) | (unsigned int)u;
          sw[u] = key[j];
        }
        wave_lds_order();
        unsigned long long rem = actw;
        while (rem) {
          const int i = __builtin_ctzll(rem);
          rem &= rem - 1;
          const unsigned int mw = (unsigned int)s_mtab[i * MT + lane];
          unsigned int v[VPL];
#pragma unroll
          for (int j = 0; j < VPL; ++j) v[j] = sw[(mw >> (8 * j)) & 255u];
          wave_lds_order();
#pragma unroll
          for (int j = 0; j < VPL; ++j) { key[j] = max(key[j], v[j]); sw[lane + 64 * j] = key[j]; }
          wave_lds_order();
        }
        const double pxk = s_px[kvalid ? k : 0];
        double xo[VPL];
        unsigned int tk_own = 0u;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          const unsigned int cand = (unsigned int)__builtin_amdgcn_readlane((int)(ws[j] >> 8), k & 63);
          tk_own = ((k >> 6) == j) ? cand : tk_own;
        }
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          const int u = lane + 64 * j;
          xo[j] = txrow[u < N ? u : 0];
          // a young entry's xpos is in the subject's ring row, not (necessarily) in the plane
          if (tk_own - (ws[j] >> 8) <= 7u) xo[j] = ringp[(size_t)(bR + (kvalid ? k : 0)) * 8 + ((ws[j] >> 8) & 7u)];
          xo[j] = (u == k) ? pxk : xo[j];
        }
        if (lane == 0 && kvalid) ringp[(size_t)(bR + k) * 8 + (tk_own & 7u)] = pxk;   // this slot's stamp (after the row was read)
        wave_lds_order();
#pragma unroll
        for (int j = 0; j < VPL; ++j) sx[lane + 64 * j] = xo[j];
        wave_lds_order();
        double xs[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j) xs[j] = sx[key[j] & 255u];
        wave_lds_order();
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
          const bool upd = ((key[j] ^ ws[j]) >> 8) != 0u;
          emit(k, kvalid, j, upd, upd ? (key[j] & ~255u) : ws[j], upd ? xs[j] : xo[j], tkrow, txrow,
               std::integral_constant<int, 2>{});   // with the ring: the plane complete for this column
        }
        wave_lds_order();
      }
#if DIRAL_PASS_PACKED_IO
      repack_pass(tkov);
#endif
    }
