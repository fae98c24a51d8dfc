// bv_text_row_walk_body.h -- the walk of one batchfile row by one wave, as a fragment: the body of bv_text_parse_kernel (bv_text.hip) and of
// bv_text_job_parse_kernel (bv_text_job.hip), included at the end of each.  A fragment and not a device function, because the
// compiler schedules and allocates bv_text_parse_kernel differently around an inlined call, and that kernel is to stay the code it
// was (tools/kernel_codehash.sh).  In scope where it is included, and nothing declared behind it:
//   TextParseArgs a   (bv_text_rows.h)
//   const char *row; uint32_t len        the row of file f at position p, `len` bytes with its '\n'
//   const char *row0; uint32_t len0      what CHROM, POS and REF are held to: file 0's row of the position, or the position's head
//   uint32_t r, p, f, lane               r = p * n_files + f, the row's place in rowflag
// A `return` leaves the kernel.  No include guard: it is included inside function bodies.
    // ---- CHROM \t POS \t REF \t Depth \t: one lane (they are a few bytes)
    uint32_t start = 0, ok = 1, dep = 0;
    if (lane == 0) {
        uint32_t tabs = 0, i = 0, pos_digits = 0, dep_digits = 0, ref_at = 0;
        const uint32_t lim = min(min(len, len0), kMaxPrefix);
        for (; i < lim && tabs < 3; ++i) {  // CHROM, POS, REF: byte-equal to file 0's, POS decimal
            const char c = row[i];
            if (c != row0[i] || c == '\n') { ok = 0; break; }
            if (c == '\t') { if (++tabs == 2) ref_at = i + 1; continue; }
            if (tabs == 1) {
                if (!is_digit(c) || ++pos_digits > 9) { ok = 0; break; }
            }
        }
        ok = ok && tabs == 3 && pos_digits > 0;
        if (ok) {
            for (;; ++i) {  // Depth
                if (i >= min(len, kMaxPrefix)) { ok = 0; break; }
                const char c = row[i];
                if (c == '\t') { ++i; break; }
                if (!is_digit(c) || ++dep_digits > 9) { ok = 0; break; }
                dep = dep * 10u + (uint32_t)(c - '0');
            }
            ok = ok && dep_digits > 0;
        }
        start = i;
        if (ok && f == 0)  // toupper(REF[0]), 'N' when REF is empty (SlabBuilder::commit_row)
            a.ref[p] = base_code_dev(row[ref_at] == '\t' ? 'N' : row[ref_at]);
        if (ok) atomicAdd(&a.depth[p], dep);  // (wraps as the host reader's uint32_t sum does)
        else atomicOr(&a.pstate[p], kPrefixFail);
    }
    ok = __shfl(ok, 0);
    if (!ok) return;
    start = __shfl(start, 0);

    // ---- the five per-sample columns, 64 bytes per step
    const uint32_t ns = a.fsamp[f];
    const size_t cell0 = (size_t)p * a.pitch + a.foff[f];
    const uint64_t lt = (1ull << lane) - 1ull;
    uint32_t fld = 4, tok = 0, prev_sep = 1, bad = 0, indel = 0, maxr = 0;
    for (uint32_t b = start; b < len; b += 64u) {
        const uint32_t i = b + lane;
        const bool valid = i < len;
        const char c = valid ? row[i] : '\0';
        const uint64_t T = __ballot(valid && c == '\t');
        const uint64_t S = __ballot(valid && c == ' ');
        const uint64_t SEP = T | S | __ballot(valid && c == '\n');
        const uint64_t tb = T & lt;
        const uint32_t my_fld = fld + (uint32_t)__popcll(tb);
        uint32_t my_tok;
        if (tb) {
            const uint32_t t = 63u - (uint32_t)__clzll(tb);
            my_tok = (uint32_t)__popcll(S & lt & ~((2ull << t) - 1ull));
        } else {
            my_tok = tok + (uint32_t)__popcll(S & lt);
        }
        const bool after_sep = lane ? ((SEP >> (lane - 1)) & 1ull) != 0 : prev_sep != 0;
        if (valid) {
            if (c == '\n' && i != len - 1) bad = 1;  // a line break inside the row
            if (is_sep(c)) {
                // a separator ends token my_tok of field my_fld: an empty token, a tab past field 8, a row that ends early,
                // or a column whose token count is not the file's sample count are not the strict form
                if (after_sep) bad = 1;
                if (c == ' ' && my_tok + 1u >= ns) bad = 1;
                if (c == '\t' && (my_fld >= 8u || my_tok + 1u != ns)) bad = 1;
                if (c == '\n' && (my_fld != 8u || my_tok + 1u != ns)) bad = 1;
            } else if (after_sep && my_fld <= 8u && my_tok < ns) {
                const char *t = row + i;
                const size_t cell = cell0 + my_tok;
                switch (my_fld) {
                    case 4: {  // MappingQuality
                        const int v = parse_uint_token(t, 3, 255);
                        if (v < 0) bad = 1; else a.mq[cell] = (uint8_t)v;
                        break;
                    }
                    case 5: {  // Readbases: the strand goes in at finish
                        uint8_t code;
                        if (c == '+' || c == '-') {
                            code = c == '+' ? BV_CELL_INS : BV_CELL_DEL;
                            indel = 1;
                        } else if (!is_sep(t[1])) {
                            bad = 1; code = BV_CELL_N;
                        } else if (c == 'N') {
                            code = BV_CELL_N;
                        } else {
                            code = c == 'A' ? BV_BASE_A : c == 'C' ? BV_BASE_C : c == 'G' ? BV_BASE_G : c == 'T' ? BV_BASE_T : 0xFFu;
                            if (code == 0xFFu) { bad = 1; code = BV_CELL_N; }
                        }
                        a.bs[cell] = code;
                        break;
                    }
                    case 6:  // ReadbasesQuality: one character, phred = char - 33
                        if (!is_sep(t[1])) bad = 1; else a.q[cell] = (uint8_t)(c - 33);
                        break;
                    case 7: {  // ReadPositionRank
                        const int v = parse_uint_token(t, 5, 65535);
                        if (v < 0) bad = 1; else { a.rp[cell] = (uint16_t)v; maxr = max(maxr, (uint32_t)v); }
                        break;
                    }
                    default: {  // Strand
                        const uint8_t s = c == '+' ? 0u : c == '-' ? 1u : c == '.' ? 2u : 3u;
                        if (s == 3u || !is_sep(t[1])) bad = 1; else a.st[cell] = s;
                        break;
                    }
                }
            } else if (after_sep) {
                bad = 1;  // a token beyond the sample count, or in a tenth field
            }
        }
        fld += (uint32_t)__popcll(T);
        if (T) {
            const uint32_t t = 63u - (uint32_t)__clzll(T);
            tok = t == 63u ? 0u : (uint32_t)__popcll(S & ~((2ull << t) - 1ull));
        } else {
            tok += (uint32_t)__popcll(S);
        }
        prev_sep = (uint32_t)((SEP >> 63) & 1ull);
    }
    if (fld != 8u) {  // not 9 fields: the host reader refuses the row before it looks at Depth (a skip would be wrong)
        if (lane == 0) atomicOr(&a.pstate[p], kPrefixFail);
        return;
    }
    if (__ballot(bad)) {
        if (lane == 0) atomicOr(&a.pstate[p], kTokenFail);
        return;
    }
    const bool any_indel = __ballot(indel) != 0;
    for (int o = 32; o > 0; o >>= 1) maxr = max(maxr, (uint32_t)__shfl_xor((int)maxr, o));
    if (lane == 0) {
        a.rowflag[r] = any_indel ? (uint8_t)BV_TEXT_INDEL : (uint8_t)0;
        atomicMax(&a.pmax[p], maxr);
    }
