// Internal declarations shared by the HIP kernels (pg_kernels.hip) and the C-ABI host layer (pg_abi.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/popgen_hip.h"
#include "pg_nib.h"
#include "pg_np_sum.h"
#include "pg_pair_plan.h"     // PG_XV_PLANES, PG_GROUP, PG_XV_CAP; the routes and switches of the pack-and-pair pass

#define PG_MAX_POPS 16          // populations handled by the site-statistics kernels (K3/K6 take any number)
#define PG_SITES_PER_BLOCK 1024 // sites reduced by one block of the site-statistics kernels
#define PG_ABBA_SITES_PER_BLOCK 4096   // k_abba_q: fewer, longer blocks (prologue masks + epilogue reduction per block)
#define PG_ABBA_NSUM 6
#define PG_FOURPOP_NSUM 14
// windows of up to this many sites get their float64 sums in NumPy's order (k_popdist_np, k_quartet_np): quotients and products of
// small integers sit on rounding ties of the printed digit, differences of equal means are +-0.0
#define PG_NP_MAX_SITES 256
#define PG_FLAG_MISMATCH 1      // some individual's two haplotypes differ in calledness: the diploid shortcut does not apply
#define PG_FLAG_XV_OVERFLOW 2   // a window produced more XV words than reserved
#define PG_FLAG_FUSE_STALL 4    // a wave of the fused pack kernel gave up waiting for the others (never expected: the call fails)

struct PgTask2 {                // one block of k_pairC (8 rows) / k_pairD (16 rows): circulant task, see pair_store_circ
    int32_t row0, nsub, col0, lower;   // rows row0.., columns col0, col0+1, ... (mod n), nsub = number of valid columns; lower = 2
};

struct PgSynthParams {
    uint64_t seed;
    int64_t first_site_index, scaf_len;
    int32_t n_dip, n_pops, var_thr, miss_thr;
};

// ---- launchers (all asynchronous on `st`) -----------------------------------------------------------
// Every `gt` is the resident row buffer (two slots per byte, pg_nib.h) and RS its row pitch in bytes.

// int8 rows (pitch S, slots >= n_hap read as 0) -> resident rows; resident rows -> int8 rows (pitch S, every slot of the pitch)
void pg_launch_nib_pack(hipStream_t st, const int8_t *src, int S, int n_hap, int64_t n_rows, int8_t *gt, int RS);
void pg_launch_nib_expand(hipStream_t st, const int8_t *gt, int RS, int64_t n_rows, int8_t *dst, int S);
void pg_launch_synth(hipStream_t st, int8_t *gt, int RS, int n_hap, int64_t site0, int64_t n_sites,
                     const int32_t *slot_gen_hap, PgSynthParams p);

void pg_launch_popdist_fin(hipStream_t st, const int32_t *Cmat, const int32_t *Dmat, int N, int cN, int cshift, int n_win,
                           const int32_t *pop_start, int n_pops, int min_pair_sites, double *sum_out,
                           int64_t *cnt_out, int all_diploid, const int64_t *win_lo = nullptr, const int64_t *win_hi = nullptr,
                           long long skip_upto = -1);          // windows of up to skip_upto sites are left to k_popdist_np

// pi / dxy / Fst with the sums in NumPy's pairwise order (k_popdist_np + k_popstats_np); sums / cnts: [n_win][n_pops^2] scratch
void pg_launch_popdist_np(hipStream_t st, const int32_t *Cmat, const int32_t *Dmat, int N, int cN, int cshift, int n_win,
                          const int32_t *pop_start, int n_pops, const int32_t *ref_row, const int32_t *pop_rank,
                          const int32_t *task_tree, const int32_t *trees, int max_leaves, int max_side, int min_pair_sites,
                          double min_data, int do_pairs, double *sums, int64_t *cnts, double *out, const int64_t *win_lo,
                          const int64_t *win_hi, long long max_sites);

// the same with blocks of any length, a piece of 8192 values at a time (k_popdist_np_big): trees = the blob of a full piece at full_tree
// and of every task's last piece at task_tree[task]
void pg_launch_popdist_np_big(hipStream_t st, const int32_t *Cmat, const int32_t *Dmat, int N, int cN, int cshift, int n_win,
                              const int32_t *pop_start, int n_pops, const int32_t *ref_row, const int32_t *pop_rank,
                              const int32_t *task_tree, const int32_t *trees, int full_tree, int min_pair_sites, double min_data,
                              int do_pairs, double *sums, int64_t *cnts, double *out, const int64_t *win_lo, const int64_t *win_hi,
                              long long max_sites);

void pg_launch_indpair_fin(hipStream_t st, const int32_t *Cmat, const int32_t *Dmat, int N, int cN, int cshift, int n_win,
                           const int32_t *samp_start, const int32_t *samp_rank, int n_samp, int min_pair_sites, double *sum_out,
                           int64_t *cnt_out, int mean_mode, int max_ploidy);     // max_ploidy: the most haplotypes of an individual


void pg_launch_abba(hipStream_t st, const int8_t *gt, int RS, const int64_t *win_lo, const int64_t *win_hi,
                    int n_win, int max_chunks, const int32_t *pop_start, int p1, int p2, int p3, int p4,
                    double min_data, int sel, int nsum, double *part_sums, int64_t *part_used, double *sums_out,
                    int64_t *used_out, uint32_t *flags, int64_t base, long long max_sites);

void pg_launch_popfreq(hipStream_t st, const int8_t *gt, int RS, int n_hap, const int64_t *win_lo,
                       const int64_t *win_hi, int n_win, int max_chunks, const int32_t *pop_start, int n_pops,
                       unsigned long long *l_out, unsigned long long *S_out, unsigned long long *pairsum_out,
                       uint32_t *flags, int64_t base);
void pg_launch_popfreq_ordered(hipStream_t st, const int8_t *gt, int RS, const int64_t *win_lo, const int64_t *win_hi, int n_win,
                               const int32_t *pop_start, int n_pops, const uint32_t *flags, int64_t base, double *theta_out);

void pg_launch_site_counts(hipStream_t st, const int8_t *gt, int RS, int64_t site_lo, int64_t site_hi,
                           const int32_t *pop_start, int n_pops, int32_t *cnt_out);
void pg_launch_site_target(hipStream_t st, const int32_t *cnt, int64_t n_sites, int n_pops, int target, double min_data, int as_counts,
                           int has_threshold, double threshold, double *f_out, long long *i_out, uint8_t *keep_out);

void pg_launch_hap_called(hipStream_t st, const int8_t *gt, int RS, int n_hap, const int64_t *win_lo,
                          const int64_t *win_hi, int n_win, int max_chunks, unsigned long long *out);

// ---- pairwise pipeline (pg_pair2.hip) ---------------------------------------------------------------
// the two-kernel pack path: k_pack3, k_pack2, or k_pack2 behind the presence pre-pass, as `route` says
void pg_launch_pack2(hipStream_t st, const int8_t *gt, int RS, const int64_t *win_lo, const int64_t *win_hi,
                     const int64_t *goff, const int64_t *vgoff, int n_win, int max_groups, int64_t total_groups, uint32_t *Vp,
                     int NPv, uint32_t *XV, int NP, int32_t *nw, int dip, int32_t *mismatch, uint32_t *pres, int capg, int grp,
                     PgPackRoute route, const PgPairSwitches &sw);
// the fused form of k_pack3 (PgFuseArgs, pg_pair_plan.h); launch: 0 = launched
int pg_launch_pack_fused(hipStream_t st, const int8_t *gt, int RS, const int64_t *win_lo, const int64_t *win_hi, const int64_t *goff,
                         int n_win, int64_t max_words, int64_t avg_words, uint32_t *XV, int NP, int32_t *nw, int dip, int32_t *mismatch,
                         int capg, int n_units, int32_t *Cmat);
void pg_launch_expand(hipStream_t st, const int32_t *Cmat, const int32_t *Dmat, int N, int cN, int cshift, int n_win,
                      int32_t *Cfull, int32_t *Dfull);
void pg_launch_pairC(hipStream_t st, const uint32_t *Vp, const int64_t *vgoff, int n_win, const PgTask2 *tasks, int n_tasks,
                     int NPv, int n_units, int diag, int64_t avg_wq, int32_t *Cmat);
void pg_launch_pairD(hipStream_t st, const uint32_t *XY, const int32_t *nw, const int64_t *goff, int n_win,
                     const PgTask2 *tasks, int n_tasks, int NP, int N, int64_t avg_groups, int32_t *Dmat, int capg);
// the same counts on the matrix cores (pg_pair_mfma.hip): exact MX fp4 products of the bit planes, expanded in registers, one wave per block
void pg_launch_pairC_mfma(hipStream_t st, const uint32_t *Vp, const int64_t *vgoff, int n_win, int NPv, int n_units, int diag,
                          int64_t avg_wq, int64_t max_sites, int32_t *Cmat);
void pg_launch_pairD_mfma(hipStream_t st, const uint32_t *XV, const int32_t *nw, const int64_t *goff, int n_win, int NP, int N,
                          int64_t avg_words, int64_t max_vsites, int32_t *Dmat, int capg);

// the called-count products with the planes staged through LDS, one block per window part (pg_pair_tile.hip); 0 = launched
int pg_launch_pairC_tile(hipStream_t st, const uint32_t *Vp, const int64_t *vgoff, int n_win, int NPv, int n_units, int diag,
                         int64_t avg_wq, int64_t max_sites, int32_t *Cmat);

// called counts with one wave per SIMD and up to 14 tiles per wave (pg_pair_big.hip): planes of up to 224 units
void pg_launch_pairC_big(hipStream_t st, const uint32_t *Vp, const int64_t *vgoff, int n_win, int NPv, int n_units, int diag,
                         int64_t avg_wq, int64_t max_sites, int32_t *Cmat);

void pg_launch_sample_het(hipStream_t st, const int32_t *Cmat, const int32_t *Dmat, int N, int cN, int cshift, int n_win,
                          const int32_t *samp_start, int n_samp, int min_pair_sites, double *out);
void pg_launch_hapstats(hipStream_t st, const int32_t *Cmat, const int32_t *Dmat, int N, int cN, int cshift, int n_win,
                        const int32_t *pop_start, int n_pops, int max_pop, const int32_t *order, int min_pair_sites, int diag_nan,
                        double max_dist, uint32_t *bits, size_t bits_per_window, double *out);
void pg_launch_unpack(hipStream_t st, const uint8_t *cells, int n_cols, int64_t n_rows, const int32_t *slot_src, int n_hap,
                      int8_t *gt, int RS);
void pg_launch_flag_export(hipStream_t st, int32_t *flag, double *dst);
void pg_launch_popstats(hipStream_t st, const double *sums, const int64_t *cnts, int n_win, const int32_t *pop_start,
                        int n_pops, double min_data, int do_pairs, double *out, const int64_t *win_lo = nullptr,
                        const int64_t *win_hi = nullptr, long long skip_upto = -1);

// ---- a block of whole lines through one of the tokenizer's two text slots ---------------------------------
struct pg_ctx;
struct PgLineDev;               // pg_ctx::LineSlot, PgLineRoute, PgDeflate, DevBuf: pg_ctx.h
struct PgLineRoute;
struct PgLineResult;
struct PgDeflate;
template <class T>
struct DevBuf;
// pg_tokenize.hip: the text (or its deflated members) to the device, line feeds counted behind it; the wait for the count, the line
// feeds' positions queued; the members' checksums of a block whose kernels have finished
int pg_tok_text_submit(pg_ctx *c, int slot, const char *text, int fd, int64_t file_offset, int64_t len);
int pg_tok_bgzf_submit(pg_ctx *c, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                       const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                       int64_t text_len, int64_t line_len_hint);
int pg_tok_lines(pg_ctx *c, int slot, int64_t *n_lines_out);
int pg_tok_crc_result(pg_ctx *c, int slot);
// pg_deflate.hip: the *total_d bytes of text at text_d (max_text at most) as BGZF members into D.comp, their bytes into *comp_total_d,
// queued on st; status_d (may be null): status words that cancel it when raised
int pg_deflate_queue(pg_ctx *c, hipStream_t st, PgDeflate &D, const uint8_t *text_d, const long long *total_d, int64_t max_text,
                     const long long *status_d, long long *comp_total_d);
// pg_line_slot.hip: the protocol of pg_line_slot.h carried out for the per-line routes (`who`: the entry point, for the error texts).
// c->tok_small, made on first use
int pg_small_stream(pg_ctx *c);
// len bytes device -> host on the small stream (beside the next block's kernels on the copy stream), waited for
int pg_copy_back(pg_ctx *c, void *dst, const void *src, int64_t len);
// k_rows_scan queued on st: roff = the exclusive sums of rlen over the lines, rank (may be null) = those of rlen != 0; their totals into
// status[PGL_ST_BYTES] and [PGL_ST_ROWS], PG_ST_OVERFLOW raised when the bytes exceed out_cap
void pg_rows_scan_queue(hipStream_t st, const uint32_t *rlen, int64_t n_lines, int64_t *roff, long long *status, int64_t out_cap,
                        int64_t *rank = nullptr);
// D: the route's part of the context, null with a null context
int pg_line_check_slot(pg_ctx *c, int slot, const PgLineRoute *D, const char *who, const char *config_name);
int pg_line_submit_text(pg_ctx *c, int slot, PgLineDev &S, const char *text, int fd, int64_t file_offset, int64_t len, bool last_is_newline);
// ... of text in memory, its arguments checked and its last byte read here
int pg_line_submit_plain(pg_ctx *c, int slot, PgLineDev &S, const char *text, int64_t len, const char *who);
// last_known = false: whether the text ends in a line feed is read on the device in parse (a stream synchronisation more)
int pg_line_submit_bgzf(pg_ctx *c, int slot, PgLineDev &S, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off,
                        const uint32_t *in_len, const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head,
                        int64_t head_len, int64_t text_len, int64_t line_len_hint, bool last_known, bool last_is_newline);
// everything of parse in front of the route's kernels.  *nothing_out: there is nothing for the route to queue (an empty block --
// S.L.state stays PGL_EMPTY --, or one that is the host's as it stands -- queued, S.done recorded)
int pg_line_parse_begin(pg_ctx *c, int slot, PgLineDev &S, int64_t *n_lines_out, bool *nothing_out, const char *who);
// the host's status words to the device on `st`
int pg_line_status_upload(PgLineDev &S, hipStream_t st);
// behind the route's kernels: the status words back on `st`, S.done recorded there, queued
int pg_line_parse_end(pg_ctx *c, PgLineDev &S, hipStream_t st);
// the head of collect: the state checked, S.done waited for, idle, the members' checksums.  An empty block: idle, nothing else
int pg_line_collect_wait(pg_ctx *c, int slot, PgLineDev &S, const char *who);
// a route's second render: its row buffer grown for `need` bytes of rows, its render kernels and pg_line_parse_end queued on st
typedef int (*PgLineAgain)(pg_ctx *c, int slot, int64_t need, hipStream_t st);
// all of collect but the route's out-parameters: the wait, *n_lines_out (may be null; 0 for an empty block), rows that outgrew their
// room rendered once more by `again` (null: the route's rows cannot) and waited for, the status words decoded into *R (bgzf_rows: the
// fifth word counts), a host block counted in D
int pg_line_collect(pg_ctx *c, int slot, PgLineRoute &D, PgLineDev &S, bool bgzf_rows, PgLineAgain again, int64_t *n_lines_out,
                    PgLineResult *R, const char *who);
// bytes [off, off + len) of the slot's text / the first len bytes of a row buffer -> dst; `bad`: the error's text
int pg_line_text(pg_ctx *c, int slot, int64_t off, int64_t len, uint8_t *dst, const char *bad);
int pg_line_rows(pg_ctx *c, const DevBuf<uint8_t> &B, uint8_t *dst, int64_t len, const char *bad);
int pg_line_stats(const PgLineRoute *D, int64_t *blocks_out, int64_t *host_blocks_out, const char *who);

// ---- shared device routines ---------------------------------------------------------------------------
// (np_pairwise_sum, the float64 sum in NumPy's order by one lane -- k_hapstats, k_paint --: pg_np_sum.h, which the tests also build as
// plain host code)
