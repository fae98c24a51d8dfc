// bv_record_text.hip -- VCF heads and CVG rows formatted on the device from the engine's records (bv_engine_cvg_format,
// bv_engine_vcf_format_records; include/basevar_amd_record_text.h; the contract is INTEGRATION.md section 2l).  The bytes are
// defined at the head of bv_record_text_core.h and bv_numfmt_core.h, which a CPU harness compiles too; this file is their
// schedule.
//
// A line is a sequence of items (a literal, a name, a number); one wave handles one line, lane l item 64 s + l of step s:
//   count  every lane reduces its item to registers (bv_rt_item: pointers, lengths, the number as a bv_numfmt_val) and the
//          wave sums the lengths -> the line's bytes, and the first item whose number is outside its format's domain.
//          The lengths and the refusals are summed and decided on the HOST, which waits for the counts to size the text anyway.
//   write  the same reduction (so the count rounds exactly as the write does), a wave prefix sum of the lengths places the
//          items in an LDS image of the line that is laid out as the text is modulo 16 and stored a step at a time with
//          bv_text_image.h's piece: whole 16-byte words, byte stores on the edges, every byte of the text one writer.
//          A line that came as host text is copied.  A line of more than 64 items (21 groups and more) steps again.
// The VCF heads go where bv_vcf.hip's write kernel expects the uploaded heads, with the gt characters beside them; that
// file's count / scan / write kernels then run unchanged.  No atomics, no scratch, vector stores only.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/basevar_amd_indel.h"
#include "../../include/basevar_amd_record_text.h"
#include "bv_chunk_stage.h"
#include "bv_device_text.h"
#include "bv_record_text_core.h"
#include "bv_text_image.h"

using namespace bv_impl;

static_assert(BV_RT_TXT_MAX == BV_RECORD_TEXT_NAME_MAX && BV_RT_INDEL_MAX == BV_RECORD_TEXT_INDEL_MAX, "the header restates the core's bounds");

namespace {

// a step's items behind the at most 15 bytes an earlier flush left, or a CVG row's 16 items, one of them the indel column
constexpr uint32_t kStepBytes = 64u * BV_RT_ITEM_MAX;
constexpr uint32_t kImageBytes = 16u + kStepBytes + 16u;
static_assert(15u * BV_RT_ITEM_MAX / 4u + BV_RT_INDEL_MAX <= kStepBytes, "a CVG row fits a step");  // (its other items: no name, < 68 bytes)
constexpr uint32_t kNoItem = 0xffffffffu, kBadAlt = 0xfffffffeu;

struct RtArgs {
    const bv_site_result *rec;    // [n]
    const bv_group_result *grp;   // [n][n_groups]
    const uint32_t *pos;          // [n]
    const uint8_t *ref;           // [n]
    const uint8_t *chrom, *names;
    const uint32_t *name_off;     // [n_groups + 1]
    const uint64_t *htext_off;    // [n + 1] or NULL
    const uint8_t *htext;
    const uint64_t *indel_off;    // [n + 1] or NULL
    const uint8_t *indel;
    const uint32_t *line_of;      // write: [n_out] record of output line j, or NULL: j
    uint32_t *len, *bad;          // count: [n]
    uint8_t *gt;                  // write: [n_out][4] or NULL
    uint8_t *text;                // write
    const uint64_t *text_off;     // write: [n_out + 1]
    uint32_t n, n_groups, chrom_len, cvg;
};

__device__ inline bv_rt_ctx ctx_of(const RtArgs &a, uint32_t k) {
    bv_rt_ctx c;
    c.r = a.rec + k;
    c.g = a.grp + (size_t)k * a.n_groups;
    c.names = a.names; c.name_off = a.name_off; c.chrom = a.chrom;
    c.n_groups = a.n_groups; c.chrom_len = a.chrom_len;
    c.indel = a.indel; c.indel_len = 0;
    if (a.cvg && a.indel_off) {
        c.indel = a.indel + a.indel_off[k];
        c.indel_len = min((uint32_t)(a.indel_off[k + 1] - a.indel_off[k]), BV_RT_INDEL_MAX);
    }
    c.pos = a.pos[k]; c.ref = a.ref[k];
    return c;
}

__device__ inline uint32_t host_text_bytes(const RtArgs &a, uint32_t k) { return a.htext_off ? (uint32_t)(a.htext_off[k + 1] - a.htext_off[k]) : 0u; }

__global__ __launch_bounds__(64) void bv_rt_count_kernel(RtArgs a) {
    const uint32_t k = blockIdx.x, lane = threadIdx.x;
    if (k >= a.n) return;
    const bv_rt_ctx c = ctx_of(a, k);
    // an ALT code above 3 anywhere; more ALTs than are formatted here in a line that is
    uint32_t bad_alt = 0;
    const uint32_t hl = host_text_bytes(a, k);
    for (uint32_t j = lane; j <= a.n_groups; j += 64u) {
        const uint8_t n_alt = j ? c.g[j - 1u].n_alt : c.r->n_alt;
        const uint8_t *alt = j ? c.g[j - 1u].alt : c.r->alt;
        if (n_alt > (hl ? BV_MAX_ALT : BV_RT_MAX_ALT)) bad_alt = 1;
        for (uint32_t i = 0; i < BV_MAX_ALT; ++i)
            if (i < n_alt && alt[i] > 3u) bad_alt = 1;
    }
    bad_alt = wave_sum(bad_alt);
    uint32_t total = hl, bad = kNoItem;
    if (!hl && !bad_alt) {
        const uint32_t n_items = a.cvg ? bv_rt_cvg_items(&c) : bv_rt_vcf_items(&c);
        for (uint32_t base = 0; base < n_items; base += 64u) {
            const uint32_t idx = base + lane;
            const bv_rt_item it = idx >= n_items ? bv_rt_item_empty() : a.cvg ? bv_rt_cvg_item(&c, idx) : bv_rt_vcf_item(&c, idx);
            total += wave_sum(bv_rt_item_len(&it));
            bad = min(bad, wave_min(bv_rt_item_bad(&it) ? idx : kNoItem));
        }
    }
    if (lane == 0) {
        a.len[k] = total;
        a.bad[k] = bad_alt ? kBadAlt : bad;
    }
}

__global__ __launch_bounds__(64) void bv_rt_write_kernel(RtArgs a, uint32_t n_out) {
    __shared__ __attribute__((aligned(16))) uint8_t image[kImageBytes];
    const uint32_t j = blockIdx.x, lane = threadIdx.x;
    if (j >= n_out) return;
    const uint32_t k = a.line_of ? a.line_of[j] : j;
    const bv_rt_ctx c = ctx_of(a, k);
    if (a.gt && lane < 4u) a.gt[4u * (size_t)j + lane] = bv_rt_gt_code(c.r, c.ref, lane);
    const uint64_t dst = a.text_off[j], bytes = a.text_off[j + 1u] - dst;
    if (bytes == 0) return;
    if (host_text_bytes(a, k)) {
        head_copy(a.text + dst, a.htext + a.htext_off[k], bytes, lane);
        return;
    }
    const uint32_t n_items = a.cvg ? bv_rt_cvg_items(&c) : bv_rt_vcf_items(&c);
    Piece p;
    piece_open(p, a.text, dst, bytes);
    for (uint32_t base = 0; base < n_items; base += 64u) {
        const uint32_t idx = base + lane;
        const bv_rt_item it = idx >= n_items ? bv_rt_item_empty() : a.cvg ? bv_rt_cvg_item(&c, idx) : bv_rt_vcf_item(&c, idx);
        // (the bounds hold whatever the records say by now: a name or CHROM is at most BV_RT_TXT_MAX bytes, an indel column is cut
        // to BV_RT_INDEL_MAX, a number has at most 27 characters; and the piece stores no more than the bytes counted for it)
        const uint32_t len = bv_rt_item_len(&it), incl = wave_incl_scan(len, lane);
        bv_rt_item_put(&it, image + p.fill + (incl - len));
        p.fill += (uint32_t)__shfl(incl, 63, 64);
        piece_flush(p, image, base + 64u >= n_items, lane);
    }
}

}  // namespace

// Per-engine state of the two calls: the CVG text, what the kernels read, and what the count kernel leaves
struct BvRtextState {
    DeviceText text;           // the CVG rows (the VCF lines are bv_vcf.hip's text)
    uint8_t *d_in = nullptr;   // what the kernels read: prepare()'s upload
    uint8_t *d_out = nullptr;  // len u32 [n], bad u32 [n]
    size_t in_cap = 0, out_cap = 0;
};

void bv_rtext_state_free(BvRtextState *t) {
    if (!t) return;
    (void)hipSetDevice(t->text.device);
    for (uint8_t *b : {t->text.d_text, t->d_in, t->d_out})
        if (b) (void)hipFree(b);
    delete t;
}

namespace {

// The host's checks of bv_record_lines; empty, or what is wrong
std::string check_lines(const bv_record_lines *in, bool cvg) {
    const uint32_t n = in->n_lines, G = in->n_groups;
    if (in->reserved_) return "reserved_ must be zero";
    if (in->mem_kind != BV_MEM_HOST && in->mem_kind != BV_MEM_DEVICE) return "mem_kind must be BV_MEM_HOST or BV_MEM_DEVICE";
    if (n == 0) return "";
    if (!in->records || !in->pos || !in->ref_char || !in->chrom) return "null records/pos/ref_char/chrom";
    if (G && (!in->groups || !in->group_names || !in->group_name_off)) return "null groups/group_names/group_name_off with n_groups != 0";
    if (in->chrom_len == 0 || in->chrom_len > BV_RECORD_TEXT_NAME_MAX) return "chrom_len must be 1 .. " + std::to_string(BV_RECORD_TEXT_NAME_MAX);
    for (uint32_t j = 0; j < G; ++j) {
        if (in->group_name_off[j + 1] < in->group_name_off[j]) return "group_name_off out of order at group " + std::to_string(j);
        if (in->group_name_off[j + 1] - in->group_name_off[j] > BV_RECORD_TEXT_NAME_MAX)
            return "the name of group " + std::to_string(j) + " has more than " + std::to_string(BV_RECORD_TEXT_NAME_MAX) + " bytes";
    }
    if ((in->host_text_off == nullptr) != (in->host_text == nullptr) && in->host_text_off && in->host_text_off[n] != in->host_text_off[0]) return "null host_text";
    if (!in->host_text_off && in->host_text) return "host_text without host_text_off";
    for (uint32_t k = 0; in->host_text_off && k < n; ++k) {
        if (in->host_text_off[k + 1] < in->host_text_off[k]) return "host_text_off out of order at line " + std::to_string(k);
        if (in->host_text_off[k + 1] - in->host_text_off[k] >= (1ull << 31)) return "the host text of line " + std::to_string(k) + " has 2^31 bytes or more";
    }
    if (cvg) {
        if ((in->indel_off == nullptr) != (in->indel == nullptr) && in->indel_off && in->indel_off[n] != in->indel_off[0]) return "null indel";
        if (!in->indel_off && in->indel) return "indel without indel_off";
        for (uint32_t k = 0; in->indel_off && k < n; ++k) {
            if (in->indel_off[k + 1] < in->indel_off[k]) return "indel_off out of order at line " + std::to_string(k);
            if (in->indel_off[k + 1] - in->indel_off[k] > BV_RECORD_TEXT_INDEL_MAX)
                return "the indel column of line " + std::to_string(k) + " has more than " + std::to_string(BV_RECORD_TEXT_INDEL_MAX) + " bytes: pass the row as host text";
        }
    }
    if (in->mem_kind == BV_MEM_HOST)
        for (uint32_t k = 0; k < n; ++k) {
            const bool host_text = in->host_text_off && in->host_text_off[k + 1] != in->host_text_off[k];
            const uint32_t most = host_text ? BV_MAX_ALT : BV_RT_MAX_ALT;
            for (uint32_t j = 0; j <= G; ++j) {
                const uint8_t n_alt = j ? in->groups[(size_t)k * G + j - 1].n_alt : in->records[k].n_alt;
                const uint8_t *alt = j ? in->groups[(size_t)k * G + j - 1].alt : in->records[k].alt;
                auto where = [&] { return "line " + std::to_string(k) + (j ? ", group " + std::to_string(j - 1) : std::string()); };
                if (n_alt > most) return where() + ": n_alt " + std::to_string(n_alt) + " > " + std::to_string(most) + (host_text ? "" : " (a record of four ALTs goes as host text)");
                for (uint32_t i = 0; i < n_alt; ++i)
                    if (alt[i] > 3) return where() + ": alt code " + std::to_string(alt[i]) + " above 3";
            }
        }
    return "";
}

// What the kernels read, uploaded in one piece, and the count pass over it
struct Prepared {
    RtArgs a;
    std::vector<uint32_t> len;  // [n] bytes of the line / head (of its host text, where it has one)
};

// `tallied` (CVG rows, in->indel NULL): the indel columns are those of a completed tally, read where they lie
int prepare(bv_engine *e, const std::string &who, BvRtextState *t, const bv_record_lines *in, bool cvg, hipStream_t st, Prepared *out,
            const BvIndelView *tallied = nullptr) {
    const uint32_t n = in->n_lines, G = in->n_groups;
    const bool up_rec = in->mem_kind == BV_MEM_HOST;
    const uint64_t ht_lo = in->host_text_off ? in->host_text_off[0] : 0, ht_bytes = in->host_text_off ? in->host_text_off[n] - ht_lo : 0;
    const bool indel = cvg && in->indel_off;
    const uint64_t id_lo = indel ? in->indel_off[0] : 0, id_bytes = indel ? in->indel_off[n] - id_lo : 0;
    const uint32_t name_bytes = G ? in->group_name_off[G] - in->group_name_off[0] : 0;
    size_t at = 0;
    auto place = [&at](size_t bytes) { const size_t o = at; at += up16(bytes); return o; };
    const size_t o_rec = place(up_rec ? sizeof(bv_site_result) * (size_t)n : 0), o_grp = place(up_rec ? sizeof(bv_group_result) * (size_t)n * G : 0),
                 o_pos = place(4ull * n), o_ref = place(n), o_chrom = place(in->chrom_len), o_noff = place(4ull * (G + 1)), o_names = place(name_bytes),
                 o_hoff = place(in->host_text_off ? 8ull * (n + 1) : 0), o_ht = place(ht_bytes), o_ioff = place(indel ? 8ull * (n + 1) : 0),
                 o_id = place(id_bytes), o_end = at;
    // behind the upload: what the two calls add once the counts are known (line_of u32 [n], text_off u64 [n + 1])
    const size_t o_lineof = place(4ull * n), o_toff = place(8ull * (n + 1));
    BV_HIP(e, hipSetDevice(t->text.device));
    int rc = grow_device(e, &t->d_in, &t->in_cap, at);
    if (rc == BV_OK) rc = grow_device(e, &t->d_out, &t->out_cap, 8ull * n);
    if (rc != BV_OK) return rc;
    std::vector<uint8_t> h(o_end, 0);
    if (up_rec) {
        std::memcpy(h.data() + o_rec, in->records, sizeof(bv_site_result) * (size_t)n);
        if (G) std::memcpy(h.data() + o_grp, in->groups, sizeof(bv_group_result) * (size_t)n * G);
    }
    std::memcpy(h.data() + o_pos, in->pos, 4ull * n);
    std::memcpy(h.data() + o_ref, in->ref_char, n);
    std::memcpy(h.data() + o_chrom, in->chrom, in->chrom_len);
    for (uint32_t j = 0; j <= G; ++j) reinterpret_cast<uint32_t *>(h.data() + o_noff)[j] = G ? in->group_name_off[j] - in->group_name_off[0] : 0u;
    if (name_bytes) std::memcpy(h.data() + o_names, in->group_names + in->group_name_off[0], name_bytes);
    if (in->host_text_off) {
        for (uint32_t k = 0; k <= n; ++k) reinterpret_cast<uint64_t *>(h.data() + o_hoff)[k] = in->host_text_off[k] - ht_lo;
        if (ht_bytes) std::memcpy(h.data() + o_ht, in->host_text + ht_lo, ht_bytes);
    }
    if (indel) {
        for (uint32_t k = 0; k <= n; ++k) reinterpret_cast<uint64_t *>(h.data() + o_ioff)[k] = in->indel_off[k] - id_lo;
        if (id_bytes) std::memcpy(h.data() + o_id, in->indel + id_lo, id_bytes);
    }
    BV_HIP(e, hipMemcpyAsync(t->d_in, h.data(), o_end, hipMemcpyHostToDevice, st));
    RtArgs &a = out->a;
    a.rec = up_rec ? reinterpret_cast<const bv_site_result *>(t->d_in + o_rec) : in->records;
    a.grp = up_rec ? reinterpret_cast<const bv_group_result *>(t->d_in + o_grp) : in->groups;
    a.pos = reinterpret_cast<const uint32_t *>(t->d_in + o_pos);
    a.ref = t->d_in + o_ref; a.chrom = t->d_in + o_chrom; a.names = t->d_in + o_names;
    a.name_off = reinterpret_cast<const uint32_t *>(t->d_in + o_noff);
    a.htext_off = in->host_text_off ? reinterpret_cast<const uint64_t *>(t->d_in + o_hoff) : nullptr;
    a.htext = t->d_in + o_ht;
    a.indel_off = indel ? reinterpret_cast<const uint64_t *>(t->d_in + o_ioff) : nullptr;
    a.indel = t->d_in + o_id;
    if (tallied) { a.indel_off = tallied->d_off; a.indel = tallied->d_text; }
    a.line_of = reinterpret_cast<const uint32_t *>(t->d_in + o_lineof);
    a.text_off = reinterpret_cast<const uint64_t *>(t->d_in + o_toff);
    a.len = reinterpret_cast<uint32_t *>(t->d_out); a.bad = a.len + n;
    a.gt = nullptr; a.text = nullptr;
    a.n = n; a.n_groups = G; a.chrom_len = in->chrom_len; a.cvg = cvg ? 1u : 0u;
    hipLaunchKernelGGL(bv_rt_count_kernel, dim3(n), dim3(64), 0, st, a);
    BV_HIP(e, hipGetLastError());
    std::vector<uint32_t> back(2ull * n);
    BV_HIP(e, hipMemcpyAsync(back.data(), t->d_out, 8ull * n, hipMemcpyDeviceToHost, st));
    BV_HIP(e, hipStreamSynchronize(st));
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t bad = back[n + k];
        if (bad == kBadAlt) return fail(e, BV_ERR_INVALID_ARG, who + "line " + std::to_string(k) + ": a record with more ALTs than are formatted on the device, or an alt code above 3");
        if (bad != kNoItem)
            return fail(e, BV_ERR_DATA, who + "line " + std::to_string(k) + ", field " + bv_rt_item_name(cvg, bad) + " (item " + std::to_string(bad) +
                                            "): a number outside its format's domain; such a line is passed as host text (bv_record_text_on_device)");
    }
    out->len.assign(back.begin(), back.begin() + n);
    return BV_OK;
}

int entry_checks(bv_engine *e, const std::string &who, const bv_record_lines *in, const uint64_t *line_off, bool cvg) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, who + "null engine");
    if (!in || !line_off) return fail(e, BV_ERR_INVALID_ARG, who + "null lines/line_off");
    const std::string why = check_lines(in, cvg);
    if (!why.empty()) return fail(e, BV_ERR_INVALID_ARG, who + why);
    if (in->n_lines >= (1u << 26)) return fail(e, BV_ERR_TOO_LARGE, who + "2^26 lines or more: format fewer lines a call");
    return BV_OK;
}

// bv_vcf.hip asks for the heads and gt characters of the non-empty lines, where its write kernel reads them
struct FillCtx {
    bv_engine *e;
    RtArgs a;
    uint32_t n_out;
};

int fill_heads(void *ctx_, uint8_t *d_gt, uint8_t *d_head, const uint64_t *d_head_off, hipStream_t st) {
    FillCtx *f = static_cast<FillCtx *>(ctx_);
    f->a.gt = d_gt; f->a.text = d_head; f->a.text_off = d_head_off;
    hipLaunchKernelGGL(bv_rt_write_kernel, dim3(f->n_out), dim3(64), 0, st, f->a, f->n_out);
    BV_HIP(f->e, hipGetLastError());
    return BV_OK;
}

}  // namespace

extern "C" {

int bv_record_text_on_device(const bv_site_result *record, const bv_group_result *groups, uint32_t n_groups) {
    if (!record || (n_groups && !groups)) return 0;
    return bv_rt_on_device(record, groups, n_groups) ? 1 : 0;
}

}  // extern "C"

namespace {

// bv_engine_cvg_format, and bv_engine_cvg_format_tallied with the last tally's columns
int cvg_format(bv_engine *e, const std::string &who, const bv_record_lines *in, uint64_t *line_off, void *stream_, bool from_tally) {
    int rc = entry_checks(e, who, in, line_off, true);
    if (rc != BV_OK) return rc;
    BvIndelView tally;
    if (from_tally) {
        if (in->indel || in->indel_off) return fail(e, BV_ERR_INVALID_ARG, who + "indel / indel_off must be NULL: the columns are the last tally's");
        bv_indel_view(e->indel, &tally);
        if (!tally.done) return fail(e, BV_ERR_INVALID_ARG, who + "no bv_engine_indel_tally before it");
        if (tally.n != in->n_lines)
            return fail(e, BV_ERR_INVALID_ARG, who + "the last tally has " + std::to_string(tally.n) + " rows, not n_lines = " + std::to_string(in->n_lines));
        for (uint32_t k = 0; k < in->n_lines; ++k)
            if (tally.flag[k] && !(in->host_text_off && in->host_text_off[k + 1] != in->host_text_off[k]))
                return fail(e, BV_ERR_INVALID_ARG, who + "line " + std::to_string(k) + ": the tally left its indel column to the caller, and the line brings no host text");
    }
    BvRtextState *t = text_state(e, e->rtext);
    t->text.formatted = false;
    const uint32_t n = in->n_lines;
    if (n == 0) return device_text_empty(t->text, line_off);
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    Prepared p;
    rc = prepare(e, who, t, in, true, st, &p, from_tally ? &tally : nullptr);
    if (rc != BV_OK) return rc;
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t k = 0; k < n; ++k) off[k + 1] = off[k] + p.len[k];
    rc = device_text_reserve(e, t->text, off[n]);
    if (rc != BV_OK) return rc;
    BV_HIP(e, hipMemcpyAsync(const_cast<uint64_t *>(p.a.text_off), off.data(), 8ull * (n + 1), hipMemcpyHostToDevice, st));
    p.a.line_of = nullptr;
    p.a.text = t->text.d_text;
    hipLaunchKernelGGL(bv_rt_write_kernel, dim3(n), dim3(64), 0, st, p.a, n);
    BV_HIP(e, hipGetLastError());
    BV_HIP(e, hipStreamSynchronize(st));
    std::memcpy(line_off, off.data(), 8ull * (n + 1));
    device_text_done(t->text, off[n]);
    return BV_OK;
}

}  // namespace

extern "C" {

int bv_engine_cvg_format(bv_engine *e, const bv_record_lines *in, uint64_t *line_off, void *stream) {
    return cvg_format(e, "bv_engine_cvg_format: ", in, line_off, stream, false);
}

int bv_engine_cvg_format_tallied(bv_engine *e, const bv_record_lines *in, uint64_t *line_off, void *stream) {
    return cvg_format(e, "bv_engine_cvg_format_tallied: ", in, line_off, stream, true);
}

int bv_engine_cvg_fetch(bv_engine *e, void *dst, uint64_t dst_capacity, int dst_mem_kind, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_cvg_fetch: null engine");
    return device_text_fetch(e, "bv_engine_cvg_fetch: ", "bv_engine_cvg_format", e->rtext ? &e->rtext->text : nullptr, dst, dst_capacity, dst_mem_kind, stream_);
}

int bv_engine_cvg_deflate(bv_engine *e, const uint64_t *block_off, uint32_t n_blocks, int level, uint8_t *dst, uint64_t dst_capacity,
                          uint64_t *member_off, void *stream_) {
    if (!e) return fail(nullptr, BV_ERR_INVALID_ARG, "bv_engine_cvg_deflate: null engine");
    return device_text_deflate(e, "bv_engine_cvg_deflate: ", "bv_engine_cvg_format", e->rtext ? &e->rtext->text : nullptr, block_off, n_blocks, level, dst, dst_capacity,
                               member_off, stream_);
}

int bv_engine_vcf_format_records(bv_engine *e, const bv_record_lines *in, uint64_t *line_off, void *stream_) {
    const std::string who = "bv_engine_vcf_format_records: ";
    int rc = entry_checks(e, who, in, line_off, false);
    if (rc != BV_OK) return rc;
    const uint32_t n = in->n_lines;
    bv_vcf_lines L;
    std::memset(&L, 0, sizeof L);
    L.slab = in->slab;
    if (n == 0) return bv_vcf_format_lines(e, who.c_str(), &L, nullptr, line_off, stream_);
    if (!in->site) return fail(e, BV_ERR_INVALID_ARG, who + "null site");
    // the slab and the sites are checked before anything is launched: bv_vcf.hip's checks, on lines of no heads
    // (they are repeated on the lines that remain; a call that fails here leaves the last text)
    hipStream_t st = stream_ ? (hipStream_t)stream_ : e->stream;
    BvRtextState *t = text_state(e, e->rtext);
    Prepared p;
    {
        BvKeptRows rows;
        if (!in->slab && !bv_text_kept_rows(e->text, &rows))
            return fail(e, BV_ERR_INVALID_ARG, who + "slab == NULL, and no bv_engine_text_submit has left rows on this engine");
    }
    rc = prepare(e, who, t, in, false, st, &p);
    if (rc != BV_OK) {
        bv_vcf_text_drop(e);  // no text is held after a refused record
        return rc;
    }
    // the lines that have text: all but the records without ALT that bring no host text
    std::vector<uint32_t> line_of, site;
    std::vector<uint64_t> head_off(1, 0);
    for (uint32_t k = 0; k < n; ++k) {
        if (p.len[k] == 0) continue;
        line_of.push_back(k);
        site.push_back(in->site[k]);
        head_off.push_back(head_off.back() + p.len[k]);
    }
    const uint32_t m = (uint32_t)line_of.size();
    if (m) BV_HIP(e, hipMemcpyAsync(const_cast<uint32_t *>(p.a.line_of), line_of.data(), 4ull * m, hipMemcpyHostToDevice, st));
    FillCtx f{e, p.a, m};
    BvVcfDeviceHeads H{head_off.data(), fill_heads, &f};
    L.site = site.data();
    L.n_lines = m;
    std::vector<uint64_t> off(m + 1, 0);
    rc = bv_vcf_format_lines(e, who.c_str(), &L, &H, off.data(), st);
    if (rc != BV_OK) return rc;
    for (uint32_t k = 0, j = 0; k < n; ++k) {
        line_off[k] = off[j];
        if (j < m && line_of[j] == k) ++j;
    }
    line_off[n] = off[m];
    return BV_OK;
}

}  // extern "C"
