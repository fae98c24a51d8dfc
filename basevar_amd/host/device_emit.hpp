// device_emit.hpp -- `bv_call --emit device`: the VCF lines of a batch's variant records and its CVG rows, written on an engine
// from the records (bv_engine_vcf_format_records, bv_engine_cvg_format_tallied) over the rows that lie there, in the steps of
// emit_records_on_device at the end.  The few records whose numbers the device does not format (BaseTypeEngine::
// record_text_on_device: a NaN AF), or whose place is not the batch's first CHROM and one REF character, or whose row the tally
// left to the caller, are formatted here and go in as host text, with the tally's column where it made one.
// Part of call_pipeline.hpp, which includes it behind Batch and CallContext.
#pragma once

#include "indel_tokens.hpp"

namespace bvamd {

// Where a batch's '+SEQ' / '-SEQ' tokens are for bv_engine_indel_tally, and how one row's reach the host after all
struct IndelTokenSource {
    bv_indel_tokens tok{};           // the tally's tokens ...
    bool in_pileup = false;          // ... or none: those of the engine's last pileup, where they lie
    std::vector<uint32_t> key;       // row i's tokens are those of pos == key[i]
    LazyTokenList *list = nullptr;   // a row's tokens come from this list, fetched when the first row asks; nullptr: they are its SiteText's
    TokenList laid_out;              // (site_texts: what `tok` points at)
    const std::vector<uint8_t> *host_read = nullptr;  // engine_list: [rows], 1 where the host reader made the record -- the list never holds its tokens, its SiteText does

    // BAM input: the tokens lie with the engine's last pileup, keyed by position; `window`: that pileup's list
    static IndelTokenSource pileup(const std::vector<SiteText> &text, LazyTokenList &window) {
        IndelTokenSource s;
        s.in_pileup = true; s.list = &window;
        for (const SiteText &st : text) s.key.push_back(st.ref_pos);
        return s;
    }
    // --indel-tokens device: they lie on `engine` since its parse, keyed by the position's index in the batch; `fetch`: that list
    static IndelTokenSource engine_list(BaseTypeEngine &engine, const Batch &b, LazyTokenList &fetch) {
        IndelTokenSource s;
        if (!b.text.empty()) s.tok = engine.text_tokens();
        s.key = b.position; s.list = &fetch; s.host_read = &b.host_read;
        return s;
    }
    // ... else the SiteTexts have them: handed over as host descriptors keyed by the row's index in the batch
    static IndelTokenSource site_texts(const std::vector<SiteText> &text, int threads) {
        IndelTokenSource s;
        s.laid_out = TokenList::from_site_texts(text, threads);
        s.tok = s.laid_out.as_indel_tokens();
        for (size_t i = 0; i < text.size(); ++i) s.key.push_back((uint32_t)i);
        return s;
    }
    bool host_read_row(size_t i) const { return host_read && (*host_read)[i]; }
    std::vector<std::string> row_tokens(size_t i, const SiteText &st) const { return list ? list->get().of(key[i]) : st.indel_tokens; }
};

// The indel columns of the batch's rows, tallied and left on the engine for bv_engine_cvg_format_tallied
struct IndelTally {
    std::vector<uint64_t> col_off;  // [rows + 1]
    std::vector<uint8_t> flagged;   // [rows]: 1 where the tally left the row to the caller
    IndelTally(BaseTypeEngine &engine, const IndelTokenSource &src, const std::vector<SiteText> &text) : engine_(engine), src_(src), text_(text) {
        col_off = engine.indel_tally(src.in_pileup ? nullptr : &src.tok, src.key, flagged);
    }
    // the column of a row the host formats: the tally's, fetched once if there is such a row
    std::string host_column(size_t i) {
        if (src_.host_read_row(i)) return indel_string(text_[i].indel_tokens);
        if (flagged[i]) return indel_string(src_.row_tokens(i, text_[i]));
        if (col_off[i + 1] == col_off[i]) return std::string();
        if (columns_.empty()) { columns_.resize(col_off.back()); engine_.indel_fetch(&columns_[0], col_off.back()); }
        return columns_.substr(col_off[i], col_off[i + 1] - col_off[i]);
    }
private:
    BaseTypeEngine &engine_;
    const IndelTokenSource &src_;
    const std::vector<SiteText> &text_;
    std::string columns_;
};

// What the two format calls take: the CVG rows of every record, the VCF lines of the variant ones
struct EmitPlan {
    std::string chrom, names;  // ("-" and no group where a name does not fit: every line is host text then, and no name is looked at)
    std::vector<uint32_t> name_off, pos, vpos, vidx, site;  // vidx: the VCF line's record in the batch; site: its row on the engine
    uint32_t n_groups = 0;
    std::string ref, vref, cvg_host, vcf_host;
    std::vector<uint64_t> cvg_host_off, vcf_host_off;
    std::vector<bv_site_result> vrec;
    std::vector<bv_group_result> vgrp;
    uint64_t lines_host_formatted = 0, indel_columns_host = 0;  // records the predicate refused; host-text rows with an indel column other than "."

    bv_record_lines lines(const bv_site_result *records, const bv_group_result *groups, size_t n, bool vcf, const bv_slab *slab) const {
        bv_record_lines in;
        std::memset(&in, 0, sizeof in);
        in.mem_kind = BV_MEM_HOST;
        in.chrom = chrom.data(); in.chrom_len = (uint32_t)chrom.size();
        in.n_groups = n_groups; in.group_names = names.data(); in.group_name_off = name_off.data();
        in.records = records; in.groups = n_groups ? groups : nullptr; in.n_lines = (uint32_t)n;
        in.pos = (vcf ? vpos : pos).data(); in.ref_char = (vcf ? vref : ref).data();
        in.host_text = (vcf ? vcf_host : cvg_host).data(); in.host_text_off = (vcf ? vcf_host_off : cvg_host_off).data();
        in.slab = slab; in.site = vcf ? site.data() : nullptr;
        return in;
    }
    bv_record_lines vcf_lines(const bv_slab *slab) const { return lines(vrec.data(), vgrp.data(), vrec.size(), true, slab); }
    bv_record_lines cvg_lines(const BaseTypeBatch &result) const { return lines(result.sites.data(), result.groups.data(), pos.size(), false, nullptr); }
};

// Which rows the host formats -- a record `fits` refuses (or one outside the batch's first CHROM, or without its one REF
// character), a row the tally flagged, a host-read row with tokens (`host_read`: IndelTokenSource's, may be nullptr) -- and their
// text, with host_column(i) for the indel column.  Record i is row first_row + i on the engine.  Host code: no engine call but
// what host_column makes.  `text` has a row at least.
template <class Fits, class HostColumn>
EmitPlan plan_record_lines(const std::vector<std::string> &group_names, const std::vector<SiteText> &text, const BaseTypeBatch &result, uint32_t first_row,
                           const std::vector<uint8_t> &flagged, const std::vector<uint8_t> *host_read, int threads, Fits fits, HostColumn host_column) {
    EmitPlan p;
    const size_t n = text.size();
    const uint32_t G = (uint32_t)group_names.size();
    const std::string &chrom = text[0].ref_id;
    p.name_off.assign(1, 0);
    for (const std::string &g : group_names) { p.names += g; p.name_off.push_back((uint32_t)p.names.size()); }
    bool names_fit = !chrom.empty() && chrom.size() <= BV_RECORD_TEXT_NAME_MAX;
    for (const std::string &g : group_names) names_fit = names_fit && g.size() <= BV_RECORD_TEXT_NAME_MAX;
    p.chrom = names_fit ? chrom : "-";
    p.n_groups = names_fit ? G : 0u;
    // the predicate on the run's host threads
    std::vector<uint8_t> on_device(n, 0);
    parallel_ranges(n, threads, [&](size_t, size_t lo, size_t hi) {
        for (size_t i = lo; i < hi; ++i)
            on_device[i] = names_fit && text[i].ref_id == chrom && text[i].ref_base.size() == 1 && fits(result.sites[i], G ? &result.group(i, 0) : nullptr, G);
    });
    p.pos.resize(n);
    p.ref.assign(n, 'N');
    p.cvg_host_off.assign(1, 0);
    p.vcf_host_off.assign(1, 0);
    for (size_t i = 0; i < n; ++i) {
        const SiteText &st = text[i];
        const bv_site_result &r = result.sites[i];
        const bv_group_result *g = G ? &result.group(i, 0) : nullptr;
        p.pos[i] = st.ref_pos;
        if (st.ref_base.size() == 1) p.ref[i] = st.ref_base[0];
        if (!on_device[i]) ++p.lines_host_formatted;
        const bool host_tokens = host_read && (*host_read)[i] && !st.indel_tokens.empty();  // host text, as a flagged row
        if (!on_device[i] || flagged[i] || host_tokens) {
            const std::string column = host_column(i), row = format_cvg_line(st, r, column);
            if (!row.empty() && !column.empty() && column != ".") ++p.indel_columns_host;
            p.cvg_host += row;
        }
        p.cvg_host_off.push_back(p.cvg_host.size());
        if (!result.has_variant(i)) continue;
        p.vrec.push_back(r);
        if (G) p.vgrp.insert(p.vgrp.end(), g, g + G);
        p.vpos.push_back(st.ref_pos);
        p.vref.push_back(p.ref[i]);
        p.vidx.push_back((uint32_t)i);
        p.site.push_back(first_row + (uint32_t)i);
        if (!on_device[i]) p.vcf_host += format_vcf_head(st, r, g, group_names);
        p.vcf_host_off.push_back(p.vcf_host.size());
    }
    return p;
}

// The VCF lines: line j of the batch is text[vcf_line_off[j] .. vcf_line_off[j + 1]) and belongs to record vcf_record[j].  The
// text comes back as BGZF members deflated on the engine too (a *.vcf.gz, at --deflate-level) or as it is.
inline void write_vcf_on_device(const CallContext &ctx, BaseTypeEngine &engine, Batch &b, const EmitPlan &plan, const bv_slab *slab) {
    const std::vector<uint64_t> off = engine.vcf_format_records(plan.vcf_lines(slab));
    b.vcf_line_off.assign(1, 0);
    for (size_t k = 0; k < plan.vrec.size(); ++k) {
        if (off[k + 1] == off[k]) continue;  // (no ALT: format_vcf_line writes nothing)
        b.vcf_record.push_back(plan.vidx[k]);
        b.vcf_line_off.push_back(off[k + 1]);
    }
    b.counts.vcf_lines_device = b.vcf_record.size();
    const uint64_t total = off.back();
    if (total && ctx.vcf_gz) {
        const std::vector<uint64_t> block_off = bgzf_block_table(total);
        const size_t nb = block_off.size() - 1;
        b.vcf_members.resize(total + 31 * nb);
        b.vcf_member_off.assign(nb + 1, 0);
        engine.vcf_deflate(total, block_off.data(), (uint32_t)nb, b.vcf_members.data(), b.vcf_member_off.data(), ctx.deflate_level);
        b.vcf_members.resize(b.vcf_member_off[nb]);
    } else if (total) {
        b.vcf_text.resize(total);
        engine.vcf_fetch(&b.vcf_text[0], total);
    }
}

// The CVG rows of every record, around the tally's columns; the text comes back as it is
inline void write_cvg_on_device(BaseTypeEngine &engine, Batch &b, const EmitPlan &plan, const std::vector<uint64_t> &col_off) {
    const std::vector<uint64_t> coff = engine.cvg_format_tallied(plan.cvg_lines(b.result));
    b.cvg_device = true;
    b.cvg_text.resize(coff.back());
    if (coff.back()) engine.cvg_fetch(&b.cvg_text[0], coff.back());
    for (size_t i = 0; i < plan.pos.size(); ++i)
        if (coff[i + 1] != coff[i] && plan.cvg_host_off[i + 1] == plan.cvg_host_off[i]) {
            ++b.counts.cvg_lines_device;
            if (col_off[i + 1] != col_off[i]) ++b.counts.indel_columns_device;
        }
}

// Record i of the batch is row first_row + i of `slab`, or, with slab == nullptr, of the rows the engine's text submit kept.
inline void emit_records_on_device(const CallContext &ctx, BaseTypeEngine &engine, Batch &b, const IndelTokenSource &src, const bv_slab *slab, uint32_t first_row) {
    b.emit_device = true;
    if (b.text.empty()) return;
    IndelTally tally(engine, src, b.text);
    const EmitPlan plan = plan_record_lines(ctx.group_names, b.text, b.result, first_row, tally.flagged, src.host_read, ctx.threads,
                                            BaseTypeEngine::record_text_on_device, [&](size_t i) { return tally.host_column(i); });
    b.counts.lines_host_formatted = plan.lines_host_formatted;
    b.counts.indel_columns_host = plan.indel_columns_host;
    // the VCF lines first: on BAM input the slab's rows are the pileup's, which the next window overwrites
    write_vcf_on_device(ctx, engine, b, plan, slab);
    write_cvg_on_device(engine, b, plan, tally.col_off);
}

}  // namespace bvamd
