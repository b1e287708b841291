/* popgen_hip.h -- C ABI of libpopgen_hip.so, the MI355X (gfx950) engine behind the per-window
 * statistics path of simonhmartin/genomics_general.
 *
 * The reference has no FFI: its CLI drivers call genomics.py functions directly.  Each entry point
 * below names the reference call site(s) it replaces (paths relative to the reference root); the
 * ctypes binding a maintainer would add is shown in INTEGRATION.md and lives in
 * genomics_general_amd/_lib.py.
 *
 * Conventions
 *   - plain C, no C++ types, no exceptions across the boundary;
 *   - every function returns 0 on success, a negative pg_status on failure; the message for the last
 *     failure on the calling thread is pg_last_error();
 *   - the caller owns every host array passed in or out; the library owns all device memory of a ctx
 *     and frees it in pg_ctx_destroy;
 *   - a ctx is bound to one device and is not thread-safe; distinct ctxs may be used from distinct threads;
 *   - allele codes are one-hot int8: A=1 C=2 G=4 T=8, 0 = missing (anything that is not ACGT);
 *   - genotype blocks are site-major: gt[site][hap], haplotypes in *device slot order*, which the host
 *     chooses (populations contiguous, haplotypes of one individual adjacent);
 *   - a window is a half-open range [lo, hi) of site indices in the ctx's resident site buffer.
 */
#ifndef POPGEN_HIP_H
#define POPGEN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_ABI_VERSION 1

typedef struct pg_ctx pg_ctx;

enum pg_status {
    PG_OK = 0,
    PG_ERR_ARG = -1,       /* bad argument / precondition */
    PG_ERR_HIP = -2,       /* HIP runtime error (message carries hipGetErrorString) */
    PG_ERR_NODEV = -3,     /* no usable GPU */
    PG_ERR_PARSE = -4,     /* malformed .geno text */
    PG_ERR_RCCL = -5,      /* RCCL error */
    PG_ERR_STATE = -6      /* call made in the wrong state (e.g. no samples set) */
};

/* genotype text formats, reference `-f/--genoFormat` (popgenWindows.py:205, genomics.py:390-396) */
enum pg_geno_format { PG_FMT_PHASED = 0, PG_FMT_PAIRS = 1, PG_FMT_HAPLO = 2, PG_FMT_DIPLO = 3 };
/* OR'ed into pg_encode_text's fmt: a cell may hold FEWER alleles than its column's ploidy (the remaining slots stay missing) --
 * rows tokenised once under the widest layout of a file whose ploidy changes along it (--inferPloidy, genomics.py:1108-1111). */
#define PG_FMT_NARROW_OK 0x100

/* kernels whose HIP-event timings pg_kernel_time reports */
enum pg_kernel_id { PG_K_PACK = 0, PG_K_PAIRWISE = 1 /* the called-count kernel (k_pairC*) */, PG_K_POPDIST_FIN = 2,
                    PG_K_SITESTATS = 3, PG_K_SYNTH = 4, PG_K_PAIRD = 5 /* the difference-count kernel (k_pairD*) */,
                    PG_K_INDPAIR_FIN = 6, PG_K_RESULT_D2H = 7 /* copy of a large result table back to the host (indPair means) */,
                    PG_K_ORDERED = 8 /* k_popfreq_ordered: thetaPi as the reference's site-by-site sum */,
                    PG_K_PAINT = 9 /* k_paint: distPaint.py's decision */, PG_K_PAINT_CALLED = 10 /* k_hap_called as pg_paint runs it: the
                    individuals' own called counts */, PG_K_COUNT_ = 11 };

int pg_abi_version(void);
const char *pg_last_error(void);

/* ---- device / context -------------------------------------------------------------------------- */
int pg_device_count(int *n_out);
int pg_ctx_create(pg_ctx **out, int device);
int pg_ctx_destroy(pg_ctx *ctx);
int pg_sync(pg_ctx *ctx);

/* Haplotype -> population / individual maps in device slot order.
 * Replaces the groups/sampleNames arrays of the Alignment built by genomics.genoToAlignment
 * (genomics.py:1101-1127) and SampleData.getPop (genomics.py:1282-1286).
 * hap_pop[h] in [0,n_pops) or -1 (no population); slots of one population must be contiguous and
 * populations must appear in increasing id order, -1 slots last.  hap_sample[h] = individual index in
 * [0,n_samples); slots of one individual must be contiguous. */
int pg_set_samples(pg_ctx *ctx, int n_hap, const int32_t *hap_pop, const int32_t *hap_sample, int n_pops);

/* The order the reference's float64 sums run in (optional; identity after pg_set_samples).  pop_row_order[slots in populations]:
 * for each population the slots of its haplotypes in the order of the Alignment's rows (haplotype names sorted,
 * genomics.py:1122), concatenated in population order; pop_name_rank[n_pops]: the position of each population among np.unique's
 * sorted labels (genomics.py:965).  pg_popdist_stats then forms every np.nanmean of genomics.py:976-992 over the flattened block in
 * NumPy's pairwise-summation order -- pi / dxy / Fst equal the reference's to the last bit (populations of up to a few hundred
 * haplotypes; beyond, upper-triangle sums in a fixed tree: equal within 1e-15). */
int pg_set_reference_order(pg_ctx *ctx, const int32_t *pop_row_order, const int32_t *pop_name_rank);

/* rank[n_samples]: of an individual pair, the one with the smaller rank supplies the ROWS of the haplotype block whose np.nanmean
 * pg_indpairdist_mean forms (genomics.py:946-947: `out[s][t]`, rows = the haplotypes of s; a 2 x 2 block added up row by row).
 * popgenWindows.py reads `pairDistDict[i][j]` with i before j in sorted names (popgenWindows.py:55-57), distMat.py in the order of
 * its samples (distMat.py:44-45).  Slot order after pg_set_samples. */
int pg_set_sample_rank(pg_ctx *ctx, const int32_t *rank);

/* Which windows get their float64 sums in NumPy's order (pg_popdist_stats, pg_abbababa, pg_fourpop): 0 = those of up to 256 sites (PG_NP_MAX_SITES)
 * (default: where the last bit shows in the printed digits), 1 = all (a caller that found a value of a long window within reach of
 * a rounding tie asks again for that window: cli.py), 2 = none (fixed reduction trees, within 1e-15). */
int pg_set_sum_order(pg_ctx *ctx, int mode);

/* The pairwise-summation tree of n values as the NumPy-order kernels walk it (no device needed): out[0 .. *len) =
 * { L, n_inner, n_levels, run_offset[L + 1], node_left[n_inner], node_right[n_inner], level_start[n_levels + 1] }; runs of at most
 * 128 values (slots 0 .. L - 1), inner node k (slot L + k) = slot node_left[k] + slot node_right[k], the inner nodes ordered by
 * height, the root last.  *len is set even when cap is too small. */
int pg_np_tree(int n, int32_t *out, int64_t cap, int64_t *len);

/* ---- resident site buffer ------------------------------------------------------------------------ */
int pg_reserve_sites(pg_ctx *ctx, int64_t n_sites);
/* pg_reserve_sites for a large reservation (>= 4 GiB) with a choice of physical placement: up to max_trials (<= 8) allocations are
 * held together, the regular pack + pair path is timed on each while it is still empty, the fastest is kept (the pack kernel's
 * time moves by +-6 % with the pages behind the rows; the probe predicts it).  probe_ms_out[max_trials] (may be NULL) receives the
 * probe times, *n_trials_out the number of candidates, *chosen_out the index kept.  Smaller reservations, or when memory does not
 * hold two candidates beside the scratch budget: exactly pg_reserve_sites. */
int pg_reserve_sites_tuned(pg_ctx *ctx, int64_t n_sites, int max_trials, double *probe_ms_out, int *n_trials_out, int *chosen_out);
/* The same choice for the planes the pack kernel writes (with the rows where they are, its time still moves by up to 4 % with the
 * pages behind the planes): up to max_trials (<= 8) sets of planes are held together, the regular pack + pair path over windows of
 * window_sites (<= 0: 50 000) of rows [0, n_sites) of the reservation -- empty or filled, they are only read -- is timed on each, the
 * fastest set is kept, the others released.  Candidate 0 = the planes the context holds when called.  Outputs as above
 * (probe_ms_out[max_trials]).  A choice made on the rows as they will be read is worth more than one made on empty rows: call it
 * once a long-lived data set is loaded.  Results do not depend on it; a later pass that needs larger planes allocates new ones. */
int pg_tune_planes(pg_ctx *ctx, int64_t n_sites, int64_t window_sites, int max_trials, double *probe_ms_out, int *n_trials_out,
                   int *chosen_out);
/* Copy gt[n_sites][n_hap] (tightly packed rows) to sites [site_offset, site_offset+n_sites). */
int pg_upload_sites(pg_ctx *ctx, int64_t site_offset, const int8_t *gt, int64_t n_sites);
int pg_download_sites(pg_ctx *ctx, int64_t site_offset, int8_t *gt_out, int64_t n_sites);
/* ---- streamed ingestion: uploads that overlap the kernels of the previous input block ------------------------------------ */
/* Bytes per resident row (n_hap rounded up to 16; pad bytes zero).  A tokenizer / decoder that is told n_hap = this pitch
 * writes rows that pg_upload_sites_async copies in one piece. */
int pg_row_pitch(pg_ctx *ctx, int *pitch_out);
/* pg_upload_sites on the context's copy stream, returning at once: gt[n_sites] rows of row_pitch bytes (>= n_hap; == pg_row_pitch
 * for a single linear copy), which must stay valid -- page-locked (pg_host_alloc) for a real DMA -- until pg_upload_wait.  The
 * window calls of the context do not wait for it: upload block k+1 into rows the windows of block k do not touch (e.g. the
 * other half of the reserved rows), call pg_upload_wait before using them.  Replaces, together with pg_encode_text, the
 * reference's serial parse -> queue -> genoToAlignment hand-over (popgenWindows.py:386-403, 445-447, genomics.py:1101-1127). */
int pg_upload_sites_async(pg_ctx *ctx, int64_t site_offset, const int8_t *gt, int64_t n_sites, int64_t row_pitch);
/* The same for packed genotype cells (the `.pgeno` payload: cells[n_sites][n_cols], one byte per cell = first allele's one-hot
 * code | second allele's << 4): the cells cross PCIe as they are (0.5 byte per allele call of a diploid) and are expanded into
 * resident rows on the device (k_unpack; the host half of genomics.py:390-396, 74-77).  slot_src[n_hap]: 2 * column + allele
 * index (0/1) feeding each slot, -1 = slot unused. */
int pg_upload_packed_async(pg_ctx *ctx, int64_t site_offset, const uint8_t *cells, int64_t n_sites, int n_cols,
                           const int32_t *slot_src);
/* Block until every queued asynchronous upload of the context has landed. */
int pg_upload_wait(pg_ctx *ctx);

/* K0 on the device: `len` bytes of complete `.geno` data lines (no header; the last byte a line feed) are copied to the GPU
 * (page-locked staging, host threads) and tokenised there straight into resident rows row_offset .. (+ n lines): line feeds
 * located by a count / scan / write pass, one wavefront per line.  The same cell decoding as pg_encode_text (genomics.py:390-396,
 * 407-408, 74-77, 1884-1904), for the regular layout only: one separator character between cells, every column's cells of one
 * width (the widths are read off the block's first line; a wanted column's width must be what its ploidy says, so a file of mixed
 * ploidy -- narrower cells for its haploid samples -- is regular too), no comment or blank lines in the block.  *ok_out = 1 when the layout was regular and the rows
 * are valid; 0 otherwise (nothing may be assumed about the rows: tokenise the block with pg_encode_text and upload it).
 * Outputs: pos_out[row_capacity] the positions; the scaffold runs of the block as (first row, offset and length of the scaffold
 * token in text), sorted by row, run_capacity entries each (*ok_out = 0 when there are more).  Call pg_count_lines first to
 * reserve the rows.  Blocks on the copy stream. */
int pg_tokenize_text(pg_ctx *ctx, const char *text, int64_t len, int fmt, int n_cols, int max_ploidy, const int32_t *col_slot,
                     const int32_t *col_ploidy, int64_t row_offset, int64_t *pos_out, int64_t row_capacity, int64_t *run_row_out,
                     int64_t *run_off_out, int32_t *run_len_out, int64_t run_capacity, int64_t *n_rows_out, int64_t *n_runs_out,
                     int *ok_out);
/* The same for `len` bytes at offset file_offset of an open file (plain text on disk): the staging threads pread() the text from
 * the page cache straight into their page-locked buffers, so the block never has to be mapped, faulted in or walked by the host.
 * Offsets in run_off_out are relative to file_offset. */
int pg_tokenize_file(pg_ctx *ctx, int fd, int64_t file_offset, int64_t len, int fmt, int n_cols, int max_ploidy,
                     const int32_t *col_slot, const int32_t *col_ploidy, int64_t row_offset, int64_t *pos_out, int64_t row_capacity,
                     int64_t *run_row_out, int64_t *run_off_out, int32_t *run_len_out, int64_t run_capacity, int64_t *n_rows_out,
                     int64_t *n_runs_out, int *ok_out);
/* The device tokenizer in three steps, two blocks in flight (slot 0 / 1), for a caller that overlaps the kernels of one block with
 * the copies of the next:   parse(k) -> submit(k+1) -> collect(k).
 *   submit   text (memory when `text` is given, else `len` bytes at file_offset of fd) -> the slot's device buffer, line feeds
 *            counted behind the copies; *ok_out = 0: not the regular layout (see pg_tokenize_text), nothing submitted
 *   parse    line-feed positions, rows row_offset .. cleared, parse kernel: queued on the copy stream, not waited for; waits only
 *            for the line count (*n_rows_out); *ok_out = 0 when the rows do not fit row_capacity / the reservation
 *   collect  waits for the parse; outputs as pg_tokenize_text (offsets relative to the block's first byte) */
int pg_tokenize_submit(pg_ctx *ctx, int slot, const char *text, int fd, int64_t file_offset, int64_t len, int fmt, int n_cols,
                       int max_ploidy, const int32_t *col_slot, const int32_t *col_ploidy, int *ok_out);
int pg_tokenize_parse(pg_ctx *ctx, int slot, int64_t row_offset, int64_t row_capacity, int64_t run_capacity, int64_t *n_rows_out,
                      int *ok_out);
int pg_tokenize_collect(pg_ctx *ctx, int slot, int64_t *pos_out, int64_t pos_capacity, int64_t *run_row_out, int64_t *run_off_out,
                        int32_t *run_len_out, int64_t run_capacity, int64_t *n_rows_out, int64_t *n_runs_out, int *ok_out);
/* Packed cells (`.pgeno` with codec none: one byte per genotype) straight from the file, by the staging
 * threads of the device tokenizer: pg_stage_file brings `len` bytes at file_offset of fd to byte dst_offset of staging slot 0 / 1
 * on the device (`capacity` bytes are made sure of when dst_offset == 0; returns when the bytes have landed); pg_unpack_staged
 * queues the expansion of n_rows rows of n_cols cells at byte src_offset of the slot into resident rows row_offset .. (slot_src as
 * pg_upload_packed_async) on the copy stream; pg_stage_sync waits for that stream.  The caller alternates the slots so that the
 * expansion of one block runs while the next block crosses PCIe. */
int pg_stage_file(pg_ctx *ctx, int slot, int fd, int64_t file_offset, int64_t len, int64_t dst_offset, int64_t capacity);
int pg_unpack_staged(pg_ctx *ctx, int slot, int64_t src_offset, int64_t n_rows, int n_cols, const int32_t *slot_src, int64_t row_offset);
int pg_stage_sync(pg_ctx *ctx);
/* What the device tokenizer of this context has spent so far: wall seconds of the host -> device copies of the text (staging
 * threads start to join: the PCIe-bound part), wall seconds of everything behind them (line feeds, parse kernel, positions and
 * runs back), and the bytes of text tokenised. */
int pg_tokenize_stats(pg_ctx *ctx, double *stage_seconds_out, double *kernel_seconds_out, int64_t *bytes_out);
/* Copy n resident rows from src_row to dst_row (ranges may overlap): the rows carried over to the next block of a stream. */
int pg_move_rows(pg_ctx *ctx, int64_t src_row, int64_t dst_row, int64_t n);

/* Fill sites on device with the counter-based synthetic generator (genomics_general_amd/synth.py is
 * the specification).  Dense layout: site i is scaffold i / scaf_len, position i % scaf_len + 1.
 * slot_gen_hap[h] = generator haplotype index held by device slot h. */
int pg_synth_fill(pg_ctx *ctx, int64_t site_offset, int64_t n_sites, int64_t first_site_index, uint64_t seed,
                  int64_t scaf_len, int32_t n_dip, int32_t n_pops_gen, const int32_t *slot_gen_hap,
                  int32_t var_thr, int32_t miss_thr);

/* ---- K0: host tokenizer (no GPU needed) -------------------------------------------------------- */
/* Replaces GenoFileReader.nextSite / parseGenoLine (genomics.py:1940-1945, 1884-1904) + splitSeq /
 * forceHomo / seqArrayToNumArray (genomics.py:390-396, 407-408, 74-77) for a buffer of complete lines.
 *   buf,len      text (no header line); lines starting with '#' are skipped, an empty line ends input
 *   n_cols       number of genotype columns in the file
 *   col_slot     [n_cols][max_ploidy] device slot of each allele of each column, -1 = column/allele unused
 *   col_ploidy   [n_cols] expected ploidy of the column's cells (0 = column not wanted)
 *   gt_out       [cap_sites][n_hap] one-hot codes (rows are fully written, unused slots = 0)
 *   pos_out      [cap_sites]
 *   scaf_off/len [cap_sites] byte offset/length of the scaffold token of each row inside buf
 *   n_sites_out  rows produced.  n_threads <= 0 -> hardware concurrency.
 * Error PG_ERR_PARSE when a wanted cell does not have the width its ploidy/format implies (the
 * reference asserts "Sample ploidy doesn't match number of sequences", genomics.py:1111). */
int pg_encode_text(const char *buf, size_t len, int fmt, int n_cols, int max_ploidy, const int32_t *col_slot,
                   const int32_t *col_ploidy, int n_hap, int8_t *gt_out, int64_t *pos_out, int64_t *scaf_off,
                   int32_t *scaf_len, int64_t cap_sites, int64_t *n_sites_out, int n_threads);
/* --inferPloidy: the reference takes the ploidy of a sample in a window from the cells the window holds (genoToAlignment with
 * ploidy None, genomics.py:1108-1111; splitSeq zips them, 390-396), so the cell widths of the whole input decide.  This walks a
 * buffer of whole lines and reports the data rows at which the width of a watched column's cell changes: change_row_out[k] (index
 * among the buffer's data rows), change_width_out[k][n_cols] (the widths from that row on; unwatched columns 0).  state[n_cols]
 * carries the last row's widths from buffer to buffer (start with -1 everywhere).  *n_changes_out is the true count; when it
 * exceeds cap nothing is lost -- call again with more room (state is advanced only when all changes fitted). */
int pg_text_cell_widths(const char *buf, size_t len, int n_cols, const int32_t *col_watch, int32_t *state,
                        int64_t *change_row_out, int32_t *change_width_out, int64_t cap, int64_t *n_changes_out,
                        int64_t *n_rows_out);
/* Row indices at which the scaffold token changes (contiguous scaffold runs, the unit slidingCoordWindows
 * restarts its window on, genomics.py:2013-2017).  n_runs_out is always the true count. */
int pg_scaffold_runs(const char *buf, const int64_t *scaf_off, const int32_t *scaf_len, int64_t n_sites,
                     int64_t *run_start_out, int64_t max_runs, int64_t *n_runs_out);
/* The same on RAW text (before any tokenising): byte offsets, relative to buf, of the first data line of every run of data lines
 * ('#' lines and empty lines skipped, genomics.py:1943) that share their first field.  n_out is always the true count (call
 * again with a larger cap).  Used to plan the sharding of `--windType predefined` input, whose forward-only reader
 * (genomics.py:2112-2171) makes the windows depend on the order of the runs in the whole file. */
int pg_text_runs(const char *buf, size_t len, int64_t *starts_out, int64_t cap, int64_t *n_out);
/* Window-range cuts of the multi-GPU input plan on RAW text.  A coordinate window is a function of (scaffold, position)
 * (genomics.py:1988-2017) and the reference hands windows, not scaffolds, to its workers (popgenWindows.py:396-403, 445-447), so a
 * rank's share of the input may start and end inside a scaffold run.  pg_text_seek_pos walks the data lines of buf (offset 0 = a
 * line start) while their first field equals scaf[0..scaf_len) and their position is < pos_min.  *off_out = offset of the line
 * it stopped at, *state_out = 1 (that line is of the run and has position *pos_out >= pos_min), 0 (that line belongs to another
 * scaffold: the run is over) or -1 (end of the buffer; with whole = 0 an unterminated last line is left for the next call),
 * *rows_out = data lines walked over.  pg_text_skip_rows: offset of the data line that follows n_rows data lines (row-index cuts
 * of sites windows, genomics.py:2032-2108); *rows_out < n_rows when the buffer ends first (*off_out = len). */
int pg_text_seek_pos(const char *buf, size_t len, int whole, const char *scaf, size_t scaf_len, int64_t pos_min, int64_t *off_out,
                     int32_t *state_out, int64_t *pos_out, int64_t *rows_out);
int pg_text_skip_rows(const char *buf, size_t len, int64_t n_rows, int64_t *off_out, int64_t *rows_out);
/* CPUs the process may really use: logical CPUs, cut by the affinity mask and the cgroup CPU quota.  What the library's host
 * thread pools are sized from when PG_HOST_THREADS is not set. */
int pg_usable_cpus(void);
/* Count data rows (non-'#', non-empty) in a text buffer so the caller can size the outputs. */
int pg_count_lines(const char *buf, size_t len, int64_t *n_rows_out);

/* ---- VCF -> genotype cells (host only): the native half of the parseVCF.py drop-in ------------------------------------------- */
/* Replaces, for a buffer of complete VCF lines (header lines may be included, they are skipped), VcfSite.__init__ / getSiteType /
 * getGenotype and the per-site filters of VCF_processing/parseVCF.py:49-191, 367-377.  One output row per kept site:
 *   chars_out[cap][2 * n_sel]   the allele characters the reference would print for selected sample s at [2s], [2s+1] (missing =
 *                               `missing`, second character 0 for a haploid sample); phase_out[cap][n_sel] '/' or '|'
 *   idx_out[cap][2 * n_sel]     the allele indices behind those characters (-1 = missing); row_flag_out[cap] = 1 when some printed
 *                               allele of the row is longer than one character (its character is `missing`; a text renderer takes
 *                               the strings from REF / ALT through idx_out)
 *   pos_out, chrom_off/len, ref_off/len, alt_off/len   POS and the locations of the CHROM, REF and ALT tokens in buf
 * sel_col[n_sel]: index of each selected sample among the VCF's sample columns; sel_ploidy: its expected ploidy (1 or 2).
 * flags: PG_VCF_*.  min_qual <= 0 / max_ref_len <= 0: no such filter.  contigs: names separated by '\n', contig_mode 0 none,
 * 1 include list, 2 exclude list.  prev_chrom / prev_pos: CHROM and POS tokens of the data line before the buffer (for
 * --excludeDuplicates across blocks; NULL at the start).  n_multibase_out: printed allele calls longer than one character.
 * cap_sites = 0: only count the kept sites. */
#define PG_VCF_SKIP_INDELS 1
#define PG_VCF_KEEP_PARTIAL 2
#define PG_VCF_MISMATCH_TO_MISSING 4
#define PG_VCF_EXCLUDE_DUPLICATES 8
typedef struct pg_vcf_filter {      /* --gtf flag=X min=X max=X siteTypes=.. gtTypes=.. samples=..  (parseVCF.py:255-266, 117-131) */
    const char *flag;               /* FORMAT field, e.g. "DP" */
    double min, max;
    int site_types;                 /* bit mask 1 MONO | 2 SNP | 4 INDEL, 0 = every site type */
    int gt_types;                   /* bit mask 1 Het | 2 HomRef | 4 Missing | 8 HomAlt, 0 = every genotype type */
    const uint8_t *samples;         /* per selected sample 0/1, NULL = every sample */
} pg_vcf_filter;
int pg_encode_vcf(const char *buf, size_t len, int n_vcf_samples, int n_sel, const int32_t *sel_col, const int32_t *sel_ploidy,
                  int flags, double min_qual, int max_ref_len, const pg_vcf_filter *filters, int n_filters, const char *contigs,
                  int n_contig_bytes, int contig_mode, char missing, const char *prev_chrom, int prev_chrom_len, const char *prev_pos,
                  int prev_pos_len, uint8_t *chars_out, int8_t *idx_out, uint8_t *phase_out, uint8_t *row_flag_out, int64_t *pos_out,
                  int64_t *chrom_off, int32_t *chrom_len, int64_t *ref_off, int32_t *ref_len, int64_t *alt_off, int32_t *alt_len,
                  int64_t cap_sites, int64_t *n_sites_out, int64_t *n_multibase_out, int n_threads);
/* The `.geno` text of rows [0, n_rows) of pg_encode_vcf's outputs, as the reference prints them (VCF_processing/parseVCF.py:151-169
 * the cells, 380-383 the line: CHROM, POS[, REF when add_ref], one cell per selected sample, joined by sep): a cell = the sample's
 * allele characters joined by its phase character; in a row whose row_flag is set the cells are put together from the REF / ALT
 * strings in buf through idx.  out == NULL: only *out_len_out (the bytes the rows take) is computed. */
int pg_vcf_render_rows(const char *buf, int64_t n_rows, int n_sel, const int32_t *sel_ploidy, const uint8_t *chars, const int8_t *idx,
                       const uint8_t *phase, const uint8_t *row_flag, const int64_t *pos, const int64_t *chrom_off,
                       const int32_t *chrom_len, const int64_t *ref_off, const int32_t *ref_len, const int64_t *alt_off,
                       const int32_t *alt_len, char sep, char missing, int add_ref, uint8_t *out, int64_t out_cap,
                       int64_t *out_len_out, int n_threads);

/* ---- VCF lines -> `.geno` rows on the device (csrc/pg_vcf_dev.hip): pg_encode_vcf + pg_vcf_render_rows in one, for the regular
 * spelling of a VCF line (single tabs, POS as plain digits, QUAL and the filtered FORMAT values as plain decimals of up to 15 digits,
 * at most 16 alleles).  Replaces the same reference lines (VCF_processing/parseVCF.py:49-191, 367-370, 380-383).  A bgzipped VCF never
 * crosses PCIe as text: k_inflate writes it into the tokenizer's text slot, only the rows come back.
 *   pg_vcf_dev_config        the option set: pg_encode_vcf's arguments + the rows' separator and --addRefTrack.  *taken_out = 0 (with
 *                            *why_out, a static string): an option set the device does not take (> 8 genotype filters, > 14 000 sample
 *                            columns, ...) -- the caller stays on pg_encode_vcf.
 *   pg_vcf_dev_submit        a block of whole lines -> text slot `slot` (0 / 1): from memory, or len bytes at file_offset of fd
 *   pg_vcf_dev_submit_bgzf   the same for a block of BGZF members (table: pg_bgzf_walk; head = text the caller holds in front of them,
 *                            text_len = head + members cut behind the block's last line feed; line_len_hint = bytes of a typical line)
 *   pg_vcf_dev_parse         queues k_vcf_heads / k_vcf_cells / k_rows_scan on the block of `slot`
 *   pg_vcf_dev_collect       waits for them.  *host_line_out < 0: *out_len_out bytes of rows (*n_rows_out rows) are ready for
 *                            pg_vcf_dev_rows; else line *host_line_out of the block is one the device does not take (or the host
 *                            parser would answer with an error): the BLOCK goes to pg_encode_vcf (pg_vcf_dev_text brings its text back
 *                            when the host never had it)
 * The ingestion loop of VCF_processing/parseVCF.py's drop-in runs   parse(k) -> submit(k+1) -> collect(k) -> rows(k). */
int pg_vcf_dev_config(pg_ctx *ctx, int n_vcf_samples, int n_sel, const int32_t *sel_col, const int32_t *sel_ploidy, int flags,
                      double min_qual, int max_ref_len, const pg_vcf_filter *filters, int n_filters, const char *contigs,
                      int n_contig_bytes, int contig_mode, char missing, char sep, int add_ref, int *taken_out, const char **why_out);
/* --excludeDuplicates (parseVCF.py:367: a line against the DATA line before it): the device carries the CHROM / POS tokens of the last
 * data line from block to block itself (k_vcf_lastkey); pg_vcf_dev_set_prev hands it the key of blocks the HOST parsed before the next
 * submit (chrom == NULL: none), pg_vcf_dev_prev returns the key the block collected from `slot` started from (120 bytes each; a
 * length of -1: none; -2: the block before ended in a line the key could not hold and went to the host parser for it: the caller has that key) -- what pg_encode_vcf needs as prev_chrom / prev_pos when that block goes to it. */
int pg_vcf_dev_set_prev(pg_ctx *ctx, const char *chrom, int chrom_len, const char *pos, int pos_len);
int pg_vcf_dev_prev(pg_ctx *ctx, int slot, char *chrom_out, int *chrom_len_out, char *pos_out, int *pos_len_out);
int pg_vcf_dev_submit(pg_ctx *ctx, int slot, const char *text, int fd, int64_t file_offset, int64_t len);
int pg_vcf_dev_submit_bgzf(pg_ctx *ctx, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                           const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                           int64_t text_len, int64_t line_len_hint, int last_is_newline);
int pg_vcf_dev_parse(pg_ctx *ctx, int slot);
int pg_vcf_dev_collect(pg_ctx *ctx, int slot, int64_t *out_len_out, int64_t *n_rows_out, int64_t *host_line_out, int64_t *bgzf_len_out);
int pg_vcf_dev_rows(pg_ctx *ctx, int slot, uint8_t *dst, int64_t len);
/* `-o out.geno.gz` (`parseVCF.py ... | bgzip`, VCF_processing/README.md:33): with pg_vcf_dev_set_output(ctx, 1) the rows of a block are
 * also deflated where they lie (csrc/pg_deflate.hip: k_deflate, a wavefront per member of 65 280 bytes of rows; no end-of-file member);
 * pg_vcf_dev_collect reports the members' bytes in *bgzf_len_out (may be NULL), pg_vcf_dev_rows_bgzf copies them to dst. */
int pg_vcf_dev_set_output(pg_ctx *ctx, int bgzf_members);
int pg_vcf_dev_rows_bgzf(pg_ctx *ctx, int slot, uint8_t *dst, int64_t len);
int pg_vcf_dev_text(pg_ctx *ctx, int slot, uint8_t *dst, int64_t len);
int pg_vcf_dev_stats(pg_ctx *ctx, int64_t *blocks_out, int64_t *host_blocks_out);

/* freq.py's output rows (freq.py:98-113) formatted on all host threads: "scaffold\tposition\tcell\tcell...\n" per kept site.
 * mode 0: values = int32 [n][n_pops][4], cells "a,c,g,t"; mode 1: values = int64 [n][n_pops]; mode 2: values = double [n][n_pops]
 * printed as NumPy prints a double rounded to four decimals (nan, 0.0, 0.3333).  run_of_row[i] indexes the scaffold names
 * (names[name_off[r] .. name_off[r+1])); keep[i] == 0 drops row i (NULL keeps all).  *out_len = bytes needed; PG_ERR_ARG when that
 * exceeds out_cap. */
int pg_format_freq_rows(int mode, int64_t n_rows, int n_pops, const void *values, const int64_t *pos, const int32_t *run_of_row,
                        const char *names, const int64_t *name_off, const uint8_t *keep, char *out, int64_t out_cap, int64_t *out_len,
                        int n_threads);
/* Rows of float64 values as Python prints them: what makeDistMatString / PhylipString / NexusString (genomics.py:2288-2306) get from
 * `distArray.round(roundTo).astype(str)`.  Value j of row i = v[i * row_len + j], rounded like np.round(x, round_to) when
 * round_to >= 0 (rint(x * 10^r) / 10^r), printed as repr(float) (shortest digits that read back; fixed notation for
 * 1e-4 <= |x| < 1e16 with ".0" behind integers, else d.ddde-XX; nan / inf / -0.0), separated by sep, a line feed behind the row;
 * prefix (may be NULL): the bytes prefix[prefix_off[i] .. prefix_off[i+1]) in front of row i (taxon labels).  out == NULL: only
 * *out_len. */
int pg_format_float_rows(const double *v, int64_t n_rows, int64_t row_len, int round_to, char sep, const char *prefix,
                         const int64_t *prefix_off, char *out, int64_t out_cap, int64_t *out_len, int n_threads);

/* Inflate the independently deflated chunks of a `.pgeno` block (zlib streams; genoio.PackedWriter) on all host threads: the
 * concatenated output goes to dst_a (first len_a bytes: the block's int32 positions) and dst_b (the rest: its cells, e.g. rows of
 * the page-locked array an upload will read).  src_off / src_len locate chunk i in src, raw_len[i] is its inflated size. */
int pg_inflate_chunks(const uint8_t *src, const int64_t *src_off, const int64_t *src_len, const int64_t *raw_len, int n_chunks,
                      uint8_t *dst_a, int64_t len_a, uint8_t *dst_b, int64_t len_b, int n_threads);

/* ---- `.geno.gz` written by bgzip (BGZF: independent gzip members of at most 64 KiB of text) ----------------------------------------
 * Replaces gzip.open() in GenoFileReader.__init__ (genomics.py:1917-1919; popgenWindows.py:313 "-g input.geno.gz" is the
 * reference's normal input, its producer `parseVCF.py ... | bgzip`, VCF_processing/README.md:33).
 *
 * pg_bgzf_walk: the member table of buf[0 .. len) (RFC 1952 headers parsed; each member must carry the 'B' 'C' size subfield).  It
 * stops in front of a member that is not complete in buf, after max_members members, or once the walked members hold >= max_text
 * bytes of text (max_text <= 0: no limit).  Per member k: its deflate stream buf[in_off[k] .. + in_len[k]), ISIZE out_len[k] and
 * CRC-32 crc[k] of its trailer.  *consumed_out = bytes of buf the walked members occupy, *text_out = sum of their ISIZE. */
int pg_bgzf_walk(const uint8_t *buf, int64_t len, int64_t max_members, int64_t max_text, uint32_t *in_off, uint32_t *in_len,
                 uint32_t *out_len, uint32_t *crc, int64_t *n_members_out, int64_t *consumed_out, int64_t *text_out);
/* the members inflated by a pool of host threads (zlib): member k -> dst[out_off[k] .. + out_len[k]); crc (may be NULL) is checked.
 * The route of blocks the device tokenizer refuses and of the readers' own small reads (header line, shard cuts). */
/* ONE gzip stream (`gzip file.geno`: the reference reads it with gzip.open, popgenWindows.py:313, genomics.py:1917): nothing to run in
 * parallel, so zlib's inflate() on the reader's thread, straight into the caller's block buffer.  pg_gzip_read_lines: at least `want`
 * bytes of text (fewer only at the end of the input) extended to the next line feed, in dst[0 .. *got_out); cap > want by the
 * longest line expected; *complete_out = 0: the last line did not end inside cap (call again, append); *eof_out = 1: nothing left.
 * Concatenated members are followed; a damaged stream is PG_ERR_PARSE. */
typedef struct pg_gz pg_gz;
int pg_gzip_open(const char *path, pg_gz **out);
int pg_gzip_read_lines(pg_gz *g, uint8_t *dst, int64_t cap, int64_t want, int64_t *got_out, int *complete_out, int *eof_out);
int pg_gzip_close(pg_gz *g);
/* out4: [0] threads of the chunk-parallel decoder (0: the serial decoder, -1: it took over after a batch found no chain of chunks,
 * -2: zlib), [1] batches decoded side by side, [2] members that went on serially, [3] bytes of text handed out so far */
int pg_gzip_stats(pg_gz *g, int64_t *out4);
int pg_inflate_members(const uint8_t *comp, const uint32_t *in_off, const uint32_t *in_len, const int64_t *out_off,
                       const uint32_t *out_len, const uint32_t *crc, int64_t n_members, uint8_t *dst, int n_threads);
/* text -> BGZF, what `bgzip` writes (tools/bgzip.py; bench.py's compressed samples; tests): members of `block` bytes of text (bgzip:
 * 65280) deflated at `level` by a pool of host threads, + the empty EOF member when eof_marker != 0. */
int pg_bgzf_compress(const uint8_t *text, int64_t len, int level, int block, int eof_marker, uint8_t *out, int64_t out_cap,
                     int64_t *out_len_out, int n_threads);
/* the members inflated ON THE DEVICE (k_inflate: one wavefront per member, canonical Huffman decoding by ballot, matches copied 64
 * bytes at a time; the trailers' CRC-32 are checked when crc != NULL -- inside k_inflate as the text leaves, or by k_crc32 with PG_BGZF_CRC_FOLD=0): comp[0 .. comp_len) -> dst[0 .. sum out_len).  kernel_ms_out (may
 * be NULL): device time of the kernels.  PG_ERR_PARSE names the first damaged member. */
/* text[0 .. len) -> BGZF members (no end-of-file member) at out, deflated on the device by k_deflate -- the text crosses PCIe, so
 * this is the entry point of tests and tools (tools/bgzip.py --device); a drop-in whose text is made on the device uses
 * pg_vcf_dev_rows_bgzf.  *out_len_out: the members' bytes; kernel_ms_out (may be NULL): device time of the three kernels.
 * Replaces bgzip in `parseVCF.py ... | bgzip` (VCF_processing/README.md:33). */
int pg_bgzf_compress_device(pg_ctx *ctx, const uint8_t *text, int64_t len, uint8_t *out, int64_t out_cap, int64_t *out_len_out,
                            double *kernel_ms_out);
int pg_inflate_device(pg_ctx *ctx, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                      const uint32_t *out_len, const uint32_t *crc, int64_t n_members, uint8_t *dst, double *kernel_ms_out);
/* The submit step of the device tokenizer (pg_tokenize_submit) for a block that is still deflated -- comp[0 .. comp_len), or with
 * comp == NULL the comp_len bytes at file_offset of fd (read by the staging threads with pread) --: the members cross PCIe as they
 * are (10 - 26 x fewer bytes than their text) and are inflated into the slot's text buffer behind `head` (head_len bytes of text the
 * caller already holds: the unfinished line the previous block ended with).  The block's text = head + the members' text, cut to
 * text_len bytes (it must end with a line feed; the caller keeps what follows for the next block).  first_line: the block's first
 * line without its line feed (the cell widths are read off it).  parse / collect as for plain text; a damaged member makes
 * pg_tokenize_parse fail with PG_ERR_PARSE.  pg_tokenize_run_names reads the scaffold names of the runs pg_tokenize_collect reported
 * (offsets / lengths in the block's text) back from the device, one after the other into out: the host never had that text. */
int pg_tokenize_submit_bgzf(pg_ctx *ctx, int slot, const uint8_t *comp, int fd, int64_t file_offset, int64_t comp_len,
                            const uint32_t *in_off, const uint32_t *in_len,
                            const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                            int64_t text_len, const char *first_line, int64_t first_line_len, int fmt, int n_cols, int max_ploidy,
                            const int32_t *col_slot, const int32_t *col_ploidy, int *ok_out);
int pg_tokenize_run_names(pg_ctx *ctx, int slot, const int64_t *run_off, const int32_t *run_len, int64_t n_runs, char *out,
                          int64_t out_capacity);

/* Packed `.pgeno` input (genomics_general_amd/genoio.py: a tokenised `.geno` file kept on disk, one byte per genotype cell =
 * first allele code | second allele code << 4, in file column order): block of cells -> one-hot codes in slot order, same
 * col_slot / col_ploidy tables as pg_encode_text. */
int pg_decode_packed(const uint8_t *cells, int64_t n_rows, int n_cols, int max_ploidy, const int32_t *col_slot,
                     const int32_t *col_ploidy, int n_hap, int8_t *gt_out, int n_threads);

/* ---- K2: pairwise matrices ----------------------------------------------------------------------- */
/* Replaces Alignment.distMatrix / pairDist / numHamming (genomics.py:907-916, 903-905, 1219-1221) and
 * Alignment.pairNonNan (genomics.py:1042-1047).  For each window: D[i][j] = #sites where i and j are
 * both called and differ, C[i][j] = #sites both called; full symmetric [n_hap][n_hap] int32 matrices with
 * zero diagonal, in device slot order.  distMat[i][j] of the reference == D/C (nan when C == 0). */
int pg_pairwise(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int32_t *D_out, int32_t *C_out);

/* ---- K2+K3: population distance sums -------------------------------------------------------------- */
/* Replaces Alignment.groupDistStats (genomics.py:956-995).  For every window and every unordered
 * population pair (x<=y), in the order (0,0),(0,1),..,(0,P-1),(1,1),.. : the float64 sum of D/C over
 * haplotype pairs {i in x, j in y, i<j when x==y} with C >= max(min_pair_sites,1), and the number of such
 * pairs.  nanmean / minData / pi_s / pi_t / Fst are formed from these on the host (engine.py). */
int pg_popdist(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int min_pair_sites,
               double *sum_out, int64_t *cnt_out);

/* ---- K2+K3 with the statistics finished on the device -------------------------------------------- */
/* Replaces Alignment.groupDistStats (genomics.py:956-995) end to end: stats_out[n_win][P + (do_pairs ? P*(P-1) : 0)] =
 * pi of every population (CLI order), then (do_pairs) dxy of every pair x<y (x-major), then Fst of every pair; nan exactly
 * where the reference's nanmean_min / Fst give nan.  Same float64 operations, in the same order, as the reference. */
int pg_popdist_stats(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int min_pair_sites,
                     double min_data, int do_pairs, double *stats_out);

/* ---- K2+K6: individual-pair distance sums -------------------------------------------------------- */
/* Replaces Alignment.indPairDists (genomics.py:934-954).  For every window and unordered individual pair
 * (s<=t), (0,0),(0,1).. : sum of D/C over haplotype pairs {a in s, b in t, a<b when s==t} with
 * C >= max(min_pair_sites,1), and their number. */
int pg_indpairdist(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int min_pair_sites,
                   double *sum_out, int64_t *cnt_out);

/* The finished means instead of sums and counts (one array, half the bytes to copy back): d_out[n_win][pairs] =
 * nanmean of the haplotype-pair block of individuals (s,t) exactly as Alignment.indPairDists forms it (genomics.py:946-947):
 * s != t: sum/count (nan when no haplotype pair qualifies); s == t: the symmetric block holds every pair twice, and with
 * diag_counts_zeros != 0 (includeSameWithSame, genomics.py:940) one zero per haplotype counts as data. */
int pg_indpairdist_mean(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int min_pair_sites,
                        int diag_counts_zeros, double *d_out);
/* Deferred result tables, for loops that compute large tables back to back (bench.py's distMat shape: 40 MB per pass): with on != 0,
 * pg_indpairdist_mean returns when its kernels are done and lets the copy of the table into d_out -- which must then be page-locked
 * (pg_host_alloc), else the call behaves as before -- run on a stream of its own, beside the kernels of the following calls (two
 * device-side buffers alternate).  d_out is complete after pg_results_wait or pg_sync. */
int pg_set_deferred_results(pg_ctx *ctx, int on);
int pg_results_wait(pg_ctx *ctx);

/* The same means from pair counts the CALLER supplies: D, C as pg_pairwise writes them ([n_win][n_hap][n_hap] int32, device slot
 * order).  Pair counts are sums over sites, so the counts of disjoint parts of a window add: this is how `distMat.py --windType cat`
 * (one window = the whole input, distMat.py:284-289 / genomics.py:1949-1967) runs on several GPUs -- every rank counts its share
 * of the lines (pg_pairwise), the counts are summed across the ranks, every rank finishes the means from the sums. */
int pg_indpairdist_mean_from_counts(pg_ctx *ctx, const int32_t *D, const int32_t *C, int n_win, int min_pair_sites,
                                    int diag_counts_zeros, double *d_out);

/* ---- indHet / hapStats finished on the device (no N x N matrices leave the GPU) ------------------------------- */
/* Replaces Alignment.sampleHet (genomics.py:918-929) on the reference worker's cached distance matrix:
 * het_out[n_win][n_individuals] (slot order of the individuals) = D/C of a diploid individual's two haplotypes where bit 1 of
 * their jointly called site count is set (the reference's `len(x)==2 & C >= _minSites` precedence), nan otherwise and where
 * C < min_pair_sites (the mask a preceding groupDistStats(minSites) leaves on the cache, genomics.py:959-961; 0 = none). */
int pg_sample_het(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int min_pair_sites, double *het_out);
/* Replaces Alignment.H12stats (genomics.py:1079-1098) + distMat_to_cluster_sizes (genomics.py:1239-1261):
 * h_out[n_win][n_pops][3] = H1, H12, H2 of every population.  pop_row_order[slots in populations]: for each population the
 * slots of its haplotypes in the reference's row order (haplotype names sorted, genomics.py:1122) -- the greedy clustering
 * breaks ties by row order.  min_pair_sites as above; diag_nan != 0 when an earlier step of the reference's worker left a nan
 * diagonal on the cached matrix (groupDistStats, or indPairDists without includeSameWithSame). */
int pg_hapstats(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int min_pair_sites, int diag_nan,
                double max_dist, const int32_t *pop_row_order, double *h_out);

/* ---- K1+K4: ABBA-BABA window sums ------------------------------------------------------------------ */
/* Replaces genomics.ABBABABA(polarize=True) (genomics.py:1647-1695) with f4/D/fd/fdm/ABBA/BABA
 * (genomics.py:1409-1475, 1565-1569).  sums_out[n_win][6] = { sum f4(p1,p2,p3,p4), sum (ABBA+BABA),
 * sum f4(p1,pd,pd,p4), sum f4(pdm1,pdm2,pdm3,p4), sum ABBA, sum BABA }; sites_used_out[n_win]: the sites that entered the
 * sums, or -1 for a window without one good site (biallelic with enough data in all four populations): there the reference
 * answers sitesUsed = nan (its zip() of six names with seven values drops the 0, genomics.py:1693-1695). */
int pg_abbababa(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int p1, int p2, int p3,
                int p4, double min_data, double *sums_out, int64_t *sites_used_out);

/* ---- K1+K4': four-population window sums (fourPopWindows.py) ---------------------------------------- */
/* Replaces genomics.fourPop (genomics.py:1585-1643) and its per-site terms (genomics.py:1409-1563).
 * allele_sel chooses the allele whose frequencies p1..p4 enter the terms:
 *   PG_SEL_MINOR    default of the reference: np.argsort(all4freqs)[:,2] (genomics.py:1615)
 *   PG_SEL_POLARIZE --polarize: allele absent from P4 (genomics.py:1610)
 *   PG_SEL_FIXED    --fixed: as polarize and fixed (0 or 1) in P1, P2, P3 (genomics.py:1611-1614)
 * sums_out[n_win][14] = { sum f4, sum (ABBA+BABA), sum f4(p1,pd,pd,p4), sum f4(pdm1,pdm2,pdm3,p4), sum ABBA,
 * sum BABA, sum f4_c, sum f4_c(p1,pd,pd,p4), sum f4_c(pdm1,pdm2,pdm3,p4), sum fdh-denominator, sum
 * fdh2-denominator, sum fh-denominator, sum ABAA, sum BAAA }; sites_used_out[n_win]. */
enum pg_allele_sel { PG_SEL_MINOR = 0, PG_SEL_POLARIZE = 1, PG_SEL_FIXED = 2 };
int pg_fourpop(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int p1, int p2, int p3,
               int p4, double min_data, int allele_sel, double *sums_out, int64_t *sites_used_out);

/* ---- K1+K5: site-frequency window sums -------------------------------------------------------------- */
/* Replaces Alignment.groupFreqStats (genomics.py:1002-1028) + baseCountPi (609-616).  Sites used are those
 * with no missing call in ANY haplotype slot.  l_out[n_win]; S_out[n_win][n_pops] = #sites with >1 allele
 * in the population; pairsum_out[n_win][n_pops] = sum over sites of sum_{a<b} c_a c_b (exact integers).
 * theta_pi_out[n_win][n_pops] (may be NULL): thetaPi as the reference forms it -- Python's sum() over the per-site values
 * `pairs / (.5*N*(N-1))` in site order (genomics.py:1016-1018), a sequential float64 sum, reproduced bit for bit (Tajima's D of
 * a population of three haplotypes is that sum's rounding noise over a variance of zero). */
int pg_popfreq(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int64_t *l_out,
               int64_t *S_out, int64_t *pairsum_out, double *theta_pi_out);

/* ---- K1 raw: per-site per-population base counts ------------------------------------------------- */
/* Replaces Alignment.siteFreqs(asCounts=True) / binBaseFreqs (genomics.py:1049-1052, 592-599) for every
 * population at once: cnt_out[n_sites][n_pops][4] (A,C,G,T) for sites [site_lo, site_hi). */
int pg_site_counts(pg_ctx *ctx, int64_t site_lo, int64_t site_hi, int32_t *cnt_out);
/* freq.py's per-site finaliser on those counts (freq.py:60-105 with derivedAllele / minorAllele, genomics.py:636-669), for sites
 * [site_lo, site_hi): target 1 = derived (the last population is the outgroup), 2 = minor.  Per site and population the count of the
 * target allele (as_counts: values_out is int64[n][n_pops], 0 where the site or the population's data fail) or its frequency
 * np.around(c / n, 4) (values_out is float64[n][n_pops], NaN there; has_threshold: frequencies >= threshold become 1, the others 0);
 * a population counts when its called alleles number >= min_data (freq.py:80 compares the COUNT).  keep_out[n]: 0 for a row that
 * is all NaN / all zero (what freq.py drops without --keepNanLines). */
int pg_site_target(pg_ctx *ctx, int64_t site_lo, int64_t site_hi, int target, double min_data, int as_counts, int has_threshold,
                   double threshold, void *values_out, uint8_t *keep_out);

/* ---- site-frequency spectra (the sfs.py drop-in, cli.sfs_main; pg_sfs.hip) --------------------------------------------------------
 * Replaces sfs.py:428-496 (the per-site loop: completeness, getTargetCounts, SparseFS.add) for every spectrum at once.  A session:
 * pg_sfs_begin, any number of pg_sfs_add_*, pg_sfs_read, pg_sfs_end (pg_ctx_destroy ends an open one).
 * pg_sfs_begin: n_in ingroup populations with extents pop_ext[k] (haplotype slots + 1; a target count must stay below it); n_groups
 * spectra of group_nd[g] (1 to 4) populations group_pops[g][4] (indices into the ingroup list, the first the most significant digit
 * of the cell index); n_intervals counts per cell (1 without regions).  Per group a dense table count[cell][n_intervals] (u64) and
 * first[cell] (u64, the lowest line ordinal that touched the cell, all-ones when none did); their total size is held against the
 * scratch budget (PG_SCRATCH_GIB, pg_set_scratch_limit) before anything is allocated.  cells_out[n_groups] / on_lds_out[n_groups] (may
 * be NULL): cells per group, and whether the group is counted in LDS tables (PG_SFS_LDS=0: none is).  PG_SFS_CHUNK: sites per launch.
 * Membership of the add calls: n_runs == 0: every row counts, for interval 0.  Otherwise row i belongs to run row_run[i] and has
 * position pos[i]; run r lists the inclusive intervals [iv_start[j], iv_end[j]] -> interval id iv_id[j], j in [run_off[r],
 * run_off[r+1]); a row adds 1 per list entry that holds its position and is left out when none does.
 * ord0: the line ordinal of the call's first row (row i has ord0 + i).  ms_out (may be NULL): HIP-event time of the launches. */
int pg_sfs_begin(pg_ctx *ctx, int n_in, const int32_t *pop_ext, int n_groups, const int32_t *group_nd, const int32_t *group_pops,
                 int n_intervals, int64_t *cells_out, int32_t *on_lds_out);
/* resident rows [site_lo, site_hi): in_pops[n_in] populations of pg_set_samples, out_pop the outgroup (-1: the minor allele). */
int pg_sfs_add_sites(pg_ctx *ctx, int64_t site_lo, int64_t site_hi, uint64_t ord0, const int32_t *in_pops, int out_pop, int n_runs,
                     const int32_t *run_off, const int64_t *iv_start, const int64_t *iv_end, const int32_t *iv_id, const int32_t *row_run,
                     const int64_t *pos, double *ms_out);
/* cnt[n][n_cols][4] base counts (a freq.py table): in_cols[n_in] / out_col are columns; no completeness test (sfs.py:464-479). */
int pg_sfs_add_base_counts(pg_ctx *ctx, const int32_t *cnt, int64_t n, int n_cols, uint64_t ord0, const int32_t *in_cols, int out_col,
                           int n_runs, const int32_t *run_off, const int64_t *iv_start, const int64_t *iv_end, const int32_t *iv_id,
                           const int32_t *row_run, const int64_t *pos, double *ms_out);
/* tc[n][n_in] counts of the target allele (sfs.py:481-483). */
int pg_sfs_add_target_counts(pg_ctx *ctx, const int32_t *tc, int64_t n, uint64_t ord0, int n_runs, const int32_t *run_off,
                             const int64_t *iv_start, const int64_t *iv_end, const int32_t *iv_id, const int32_t *row_run, const int64_t *pos,
                             double *ms_out);
/* The touched cells, in no particular order: *n_out their number; with cap > 0 the first min(cap, n) of them as cell_out (index into
 * the groups' tables laid end to end), first_out, count_out[.][n_intervals].  cap == 0 only counts. */
int pg_sfs_read(pg_ctx *ctx, int64_t cap, int64_t *cell_out, uint64_t *first_out, uint64_t *count_out, int64_t *n_out);
int pg_sfs_end(pg_ctx *ctx);
/* The target allele of a site from the ingroup's totals tot4 and the outgroup's counts out4 (NULL: the minor allele, NumPy's
 * argsort()[-2] with its tie order): the device function, callable on the host.  *base_out = -1 for a site that is left out. */
int pg_sfs_target_base(const int64_t *tot4, const int64_t *out4, int *base_out);
/* k_site_counts alone over resident rows, HIP-event time without the copy to the host (tools/sfs_bench.py's yardstick). */
int pg_sfs_time_site_counts(pg_ctx *ctx, int64_t site_lo, int64_t site_hi, double *ms_out);

/* ---- nearest reference population per window and individual (distPaint.py) ---------------------------- */
/* Replaces the worker loop of distPaint.py:62-87 (which_lowest_test / which_lowest_delta, distPaint.py:26-44; Alignment.pairDist and
 * nanMask, genomics.py:903-905): the windows go through the pack and pair kernels, k_paint reads D and C in place.
 * Every sample must be haploid (PG_ERR_STATE otherwise).  ind_slot[n_ind]: the slot behind output column k.  Reference populations as a CSR list: ref_start[n_pops + 1], ref_slot[] the
 * slots of the reference individuals in the reference's order, duplicates kept (at most 64 populations and 2048 entries).  The distance
 * of a pair is D / C, nan where C < min_sites or C == 0; C of an individual with itself is its own called count.
 * mode 0 (rank-sum test): crit[n_pops][n_pops], crit[b][q] = the largest doubled rank sum 2 s of population b's values among those of b
 * and q whose p-value (scipy.stats.ranksums, alternative "less") is <= the threshold, -1 when there is none: decision = noresult as soon
 * as one comparison lies above it, else np.argmin of the populations' np.nanmean; a comparison with a nan on either side never rejects.
 * mode 1 (delta): noresult where the two smallest means are closer than delta.  Cells with a nan among their means are the caller's
 * (Python's sorted() of such a list depends on its order): *n_flagged_out of them, flag_cell_out[] = window * n_ind + column and
 * flag_means_out[][n_pops] their means, in no particular order; both arrays need room for n_win * n_ind cells.
 * decision_out[n_win][n_ind].  Kernel families PG_K_PAINT and PG_K_PAINT_CALLED. */
int pg_paint(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int n_ind, const int32_t *ind_slot, int n_pops,
             const int32_t *ref_start, const int32_t *ref_slot, int min_sites, int mode, const int64_t *crit, double delta, int noresult,
             int32_t *decision_out, int64_t *n_flagged_out, int64_t *flag_cell_out, double *flag_means_out);

/* ---- per-window column statistics (the windowStats.py drop-in, genomics_general_amd/wstats.py) --------------------------------------
 * Replaces windowStats.py:160-182: per window and column, over the non-nan values in file order, mean / median / min / max / sd /
 * sum / q5 q10 q25 q75 q90 q95 (statistic s = bit s of `mask`, in this order) as NumPy 2.2 computes them, to the last bit.
 * Host (pg_ws.cpp, no context): pg_ws_text parses a block of lines -- sel_col[k] the value field of selected column k, n_names the
 * header's value names (exact: a line must hold exactly that many) -- into vals[n_sel][pitch], pos, the scaffolds' places in the text
 * and new_run; cells of another spelling than pg_ws_core.h's regular one are listed in irr[.][4] = site, selected column (-1: the
 * position), offset, length (*n_irr_out may exceed cap_irr; *n_sites_out > cap_sites: nothing was written, come again with more room).
 * *err_out: 0, or 1 a line too short, 2 a line too long (exact), 7 not ASCII, at line *err_line_out; the sites in front of it stand.
 * pg_ws_stats_host: windows [lo, hi) of sites -> out[n_win][n_cols][12], cnt[n_win][n_cols] non-nan values, flag[n_win][n_cols] = 1
 * where min / max were asked of no value.
 * Device (pg_ws_dev.hip): pg_ws_reserve reserves the value store [n_cols][n_sites] (held against the scratch budget: PG_ERR_ARG with the
 * knob's name), pg_ws_put uploads sites [site0, site0 + n) of a column, pg_ws_stats runs k_ws_stats over the windows -- a
 * workgroup per window and column; up to lds_vals (0: the default, PG_WS_LDS_DEFAULT; 8192 at most) values are sorted in LDS, more
 * go through a radix select over global memory -- and tier_out[2] (may be NULL) counts the cells of either tier; pg_ws_copy_time
 * copies the store device to device once (the kernels' floor, tools/wstats_bench.py); pg_ws_end frees (pg_ctx_destroy ends an open one). */
#define PG_WS_LDS_DEFAULT 8192
int pg_ws_text(const char *text, int64_t len, int n_sel, const int32_t *sel_col, int n_names, int exact, int n_threads, int64_t cap_sites,
               double *vals, int64_t pitch, int64_t *pos, int64_t *scaf_off, int32_t *scaf_len, uint8_t *new_run, int64_t cap_irr,
               int64_t *irr, int64_t *n_sites_out, int64_t *n_irr_out, int64_t *n_lines_out, int *err_out, int64_t *err_line_out,
               int64_t *err_site_out);
int pg_ws_stats_host(const double *vals, int64_t pitch, int n_cols, const int64_t *lo, const int64_t *hi, int64_t n_win, uint32_t mask,
                     int n_threads, double *out, int64_t *cnt, uint8_t *flag);
int pg_ws_reserve(pg_ctx *ctx, int n_cols, int64_t n_sites);
int pg_ws_put(pg_ctx *ctx, int col, int64_t site0, const double *vals, int64_t n);
int pg_ws_stats(pg_ctx *ctx, const int64_t *lo, const int64_t *hi, int64_t n_win, uint32_t mask, int lds_vals, double *out, int64_t *cnt,
                uint8_t *flag, int64_t *tier_out, double *ms_out);
int pg_ws_copy_time(pg_ctx *ctx, double *ms_out);
/* The lines parsed on the device (k_ws_lines), a block of whole lines through text slot 0 or 1 (csrc/pg_line_slot.h: submit, parse,
 * collect).  pg_ws_dev_config: n_fields the header's fields, sel_field[n_sel] the field (>= 2) of every selected column; *taken_out = 0:
 * the host route parses.  pg_ws_dev_submit / _submit_bgzf: the text, or bgzip members that k_inflate inflates into the slot.
 * pg_ws_dev_parse: base = the sites the store holds (pg_ws_reserve(ctx, n_sel, base) first); the store grows for the block's lines and
 * the kernels are queued.  pg_ws_dev_collect: *host_line_out < 0: *n_sites_out sites stand behind base (pg_ws_reserve(ctx, n_sel, base +
 * n) takes them in), pg_ws_dev_meta gives their positions, run flags (another scaffold than the site before; the block's first site: 1)
 * and the scaffolds' places in the block's text (pg_ws_dev_text); else the block is the host route's (a line of another field count than
 * the header's, a cell outside the regular spelling, a position that is not 1 .. 18 digits, a byte that is not ASCII, a carriage
 * return, a blank line, no final line feed) and is counted in pg_ws_dev_stats' host blocks. */
int pg_ws_dev_config(pg_ctx *ctx, int n_fields, int n_sel, const int32_t *sel_field, int *taken_out);
int pg_ws_dev_submit(pg_ctx *ctx, int slot, const char *text, int64_t len);
int pg_ws_dev_submit_bgzf(pg_ctx *ctx, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                          const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                          int64_t text_len);
int pg_ws_dev_parse(pg_ctx *ctx, int slot, int64_t base, int64_t *n_lines_out);
int pg_ws_dev_collect(pg_ctx *ctx, int slot, int64_t *n_sites_out, int64_t *host_line_out, int64_t *n_lines_out);
int pg_ws_dev_meta(pg_ctx *ctx, int slot, int64_t n, int64_t *pos, uint8_t *runf, int64_t *soff, int32_t *slen);
int pg_ws_dev_text(pg_ctx *ctx, int slot, int64_t off, int64_t len, uint8_t *dst);
int pg_ws_dev_stats(pg_ctx *ctx, int64_t *blocks_out, int64_t *host_blocks_out);
int pg_ws_end(pg_ctx *ctx);

/* ---- per-haplotype called-site counts ------------------------------------------------------------ */
/* Replaces Alignment.seqNonNan (genomics.py:1038-1040) as used by distMat.py:40 (--minPerInd):
 * called_out[n_win][n_hap] = number of sites of the window at which the haplotype slot is called. */
int pg_hap_called(pg_ctx *ctx, const int64_t *win_lo, const int64_t *win_hi, int n_win, int64_t *called_out);

/* ---- measurement ------------------------------------------------------------------------------------ */
/* Accumulated HIP-event time (ms) and launch count of a kernel family since the last reset. */
int pg_kernel_time(pg_ctx *ctx, int kernel_id, double *ms_out, int64_t *launches_out);
/* Which kernel families are bracketed by events (bit k = family k, default all).  Event records between kernels cost a few
 * microseconds of GPU idle time each; a throughput run can restrict them to the family it reports. */
int pg_kernel_time_select(pg_ctx *ctx, uint32_t mask);
int pg_kernel_time_reset(pg_ctx *ctx);
/* Placement experiments (tools/pack_variance.py; not used by the drivers): device address / size of a big buffer (which: 0 resident
 * rows, 1 called plane, 2 XV planes), and a way to make its next allocation start lead_bytes behind what hipMalloc returns. */
int pg_debug_address(pg_ctx *ctx, int which, uint64_t *addr_out, uint64_t *bytes_out);
int pg_debug_place(pg_ctx *ctx, int which, uint64_t lead_bytes);
/* CU partition experiment (tools/cu_split_sweep.py; not used by the drivers): the context's compute stream on pair_cus_per_xcd
 * compute units of every XCD, the pack stream of the two-stream pipeline (PG_OVERLAP=1) on the others; 0 = plain streams. */
int pg_debug_cu_split(pg_ctx *ctx, int pair_cus_per_xcd);
/* Where the creation of the process's first context went, in seconds: [0] hipGetDeviceCount (the runtime's start-up), [1]
 * hipSetDevice + the first stream, [2] the other streams and events (tools/ctx_time.py). */
int pg_ctx_create_times(double *out3);
/* scratch budget (bytes) for per-batch bit-planes + matrices; default 48 GiB (a job that fits runs as one batch; a larger one is
 * cut into at least eight sub-batches that alternate between two slots of half the budget each) */
int pg_set_scratch_limit(pg_ctx *ctx, int64_t bytes);

/* ---- page-locked host memory ---------------------------------------------------------------------------- */
/* Output arrays handed to this library may live anywhere; when they are page-locked (allocated here) the device-to-host
 * copies of large results (pg_indpairdist, pg_pairwise) run as direct DMA at PCIe speed instead of through the runtime's
 * bounce buffer.  Plain hipHostMalloc / hipHostFree, exposed so that a host without HIP bindings can use them. */
int pg_host_alloc(size_t bytes, void **ptr_out);
int pg_host_free(void *ptr);

/* ---- C1: multi-GPU result gather (RCCL over xGMI), one process per GPU ----------------------------- */
/* Replaces the sorter/writer threads' re-ordering role (popgenWindows.py:108-157).  uid is 128 bytes. */
int pg_comm_unique_id(void *uid128_out);
int pg_comm_init(pg_ctx *ctx, int n_ranks, int rank, const void *uid128);
/* Gather count doubles from every rank into recv[n_ranks*count] on every rank (ncclAllGather). */
int pg_comm_allgather_f64(pg_ctx *ctx, const double *send, double *recv, int64_t count);
int pg_comm_barrier(pg_ctx *ctx);
int pg_comm_destroy(pg_ctx *ctx);

/* ---- `.geno` sites filtered (the filterGenotypes.py drop-in, genomics_general_amd/filtergeno.py) --------------------------------
 * Replaces filterGenotypes.py:24-58 (analysisWrapper: include / exclude, thinning per pod, siteTest, the output row) with
 * genomics.py:317-378 (Genotype), 465-575 (GenomeSite.asList / alleles / hets / nonMissing) and 742-799 (siteTest).  The per-cell and
 * per-site rules are csrc/pg_filter_core.h.  The option set: */
#define PG_FILTER_MAXPOP 32
typedef struct pg_filter_cfg {
    int32_t in_fmt, out_fmt, freq_order, force_ploidy, partial_to_missing, no_test;   /* -if 0 phased 1 diplo 2 alleles; -of 0 phased 1 diplo
                                                                                      2 bases 3 alleles 4 randomAllele 5 coded 6 count */
    int32_t n_sel, n_pops, n_cols, n_contigs, contig_mode;  /* n_cols: the header's fields; contig_mode: 1 --include given, 2 --exclude given */
    int32_t min_calls, min_alleles, min_var, has_max_het, hwe, fixed, has_pop_calls, has_pop_alleles, has_nfd;
    double max_alleles, max_het, min_freq, max_freq, nfd;    /* min_var / min_freq / max_freq 0: off */
    int64_t thin_dist, pod_size;                             /* thin_dist 0: no thinning */
    int32_t pop_calls_min[PG_FILTER_MAXPOP], pop_alleles_min[PG_FILTER_MAXPOP], pop_alleles_max[PG_FILTER_MAXPOP];
    uint32_t pop_empty;                                      /* bit k: population k has no sample */
    uint32_t pop_missing;                                    /* bit k: population k names a sample that is not selected (the
                                                                reference raises KeyError where a line reaches its filters) */
    int32_t universal_newlines;                              /* 1: a lone \r ends a line too (a file read in text mode); 0: stdin,
                                                                where \r is whitespace inside the line */
} pg_filter_cfg;
/* The tables beside it: sel_col[n_sel] the header field of each selected sample, sel_ploidy[n_sel] (-1: none given), sel_popmask[n_sel]
 * the populations (bits) a sample belongs to; contigs: n_contigs names, each ended by a 0 byte, contig_flags[n_contigs] 1 include 2 exclude.
 *
 * Host route, every spelling line.split() takes: text[0 .. len) holds data lines (universal newlines), the first of them data line
 * first_line of the file (0-based, the pods count from there); the rows -> *rows_out (free with pg_filter_free).  A line on which the
 * reference's worker raises: *err_line_out its index in the block, *err_code_out the PGF_E_* code (pg_filter_core.h), else -1 / 0. */
int pg_filter_text(const pg_filter_cfg *cfg, const int32_t *sel_col, const int32_t *sel_ploidy, const uint32_t *sel_popmask,
                   const char *contigs, int n_contig_bytes, const uint8_t *contig_flags, const char *text, int64_t len, int64_t first_line,
                   int n_threads, char **rows_out, int64_t *rows_len_out, int64_t *n_rows_out, int64_t *err_line_out, int *err_code_out);
void pg_filter_free(char *rows);
/* Device route (csrc/pg_filter_dev.hip) for the regular spelling (fields split by single tabs, the header's field count, ASCII):
 *   pg_filter_dev_config      the option set; *taken_out = 0 when the device does not take it (more than PG_FILTER_MAXPOP populations,
 *                             a header too wide for the tab table in LDS)
 *   pg_filter_dev_submit      a block of whole lines -> the tokenizer's text slot `slot` (0 / 1), its line feeds listed there; with
 *                             thinning the block must hold whole pods (first_line: the block's first data line)
 *   pg_filter_dev_submit_bgzf the same for a block still deflated (bgzip's members, pg_bgzf_walk's table; head: text in front of them):
 *                             the members cross PCIe deflated and k_inflate writes their text into the slot (no thinning: pods
 *                             cannot be cut in text the host never holds)
 *   pg_filter_dev_parse       queues k_filt_lines<0>, k_filt_thin (thinning only), the rows' scan, k_filt_lines<1> (and k_deflate)
 *   pg_filter_dev_collect     waits.  *host_line_out < 0: *rows_len_out bytes of rows (*n_rows_out) are ready for pg_filter_dev_rows
 *                             (as *bgzf_len_out bytes of BGZF members for pg_filter_dev_rows_bgzf when pg_filter_dev_set_output(ctx, 1));
 *                             rows longer than the buffer grow it and are rendered again; else line *host_line_out of the block is one
 *                             the device does not take: the block goes to pg_filter_text (pg_filter_dev_text brings its text back).
 *                             *n_lines_out: the block's line feeds
 *   pg_filter_dev_stats       blocks filtered on the device / handed to the host so far */
int pg_filter_dev_config(pg_ctx *ctx, const pg_filter_cfg *cfg, const int32_t *sel_col, const int32_t *sel_ploidy, const uint32_t *sel_popmask,
                         const char *contigs, int n_contig_bytes, const uint8_t *contig_flags, int *taken_out);
int pg_filter_dev_submit(pg_ctx *ctx, int slot, const char *text, int64_t len, int64_t first_line);
int pg_filter_dev_submit_bgzf(pg_ctx *ctx, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                              const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                              int64_t text_len, int64_t first_line);
int pg_filter_dev_set_output(pg_ctx *ctx, int bgzf_members);
int pg_filter_dev_parse(pg_ctx *ctx, int slot);
int pg_filter_dev_collect(pg_ctx *ctx, int slot, int64_t *rows_len_out, int64_t *n_rows_out, int64_t *host_line_out, int64_t *bgzf_len_out,
                          int64_t *n_lines_out);
int pg_filter_dev_rows(pg_ctx *ctx, int slot, uint8_t *dst, int64_t len);
int pg_filter_dev_rows_bgzf(pg_ctx *ctx, int slot, uint8_t *dst, int64_t len);
int pg_filter_dev_text(pg_ctx *ctx, int slot, uint8_t *dst, int64_t len);
int pg_filter_dev_stats(pg_ctx *ctx, int64_t *blocks_out, int64_t *host_blocks_out);

/* ---- `.geno` sites written as VCF rows (the genoToVCF.py drop-in, genomics_general_amd/genovcf.py) ---------------------------------
 * Replaces makeVCFline and the per-site loop of VCF_processing/genoToVCF.py:5-21, 86-90 with parseGenoLine (genomics.py:1884-1902),
 * Genotype / asCoded (317-365) and GenomeSite.alleles / asList("coded") (531-557).  The per-site and per-cell rules are
 * csrc/pg_gvcf_core.h.  The option set: */
typedef struct pg_gvcf_cfg {
    int32_t in_fmt;                                          /* -f 0 phased 1 diplo 2 pairs */
    int32_t n_sel;                                           /* output columns (-s, a name given twice counts twice) */
    int32_t n_cols;                                          /* fields of the header line */
    int32_t has_ref;                                         /* -r with at least one sequence */
    int32_t universal_newlines;                              /* 1: a file read in text mode; 0: stdin, where \r is whitespace */
} pg_gvcf_cfg;
/* The tables beside it: sel_col[n_sel] the header field of each output column (a name the header holds twice: its last field),
 * prev_same[n_cols] the field before with the same name or -1 (a line too short for the last one takes that: dict(zip(names, cells)));
 * the fasta (genoToVCF.py:55-56, parseFasta genomics.py:2256-2261) as n_seq names side by side (ref_names, name_off[n_seq + 1]), their
 * lengths seq_len[n_seq], where each begins in seq (seq_off[n_seq]) and an open-addressed table over the names (pg_gvcf_ref_table:
 * table[mask + 1], mask + 1 a power of two >= 2 n_seq and >= 4).
 *
 * Host route, every spelling line.split() takes: text[0 .. len) holds lines behind the header ('#' lines are skipped); the rows ->
 * out[0 .. out_cap) when they fit; *rows_len_out their bytes either way (3 len + 40 per line + 64 always fit).  A line on which the
 * reference dies: *err_line_out its index in the block, *err_code_out the PGG_E_* code (pg_gvcf_core.h), the rows before it written;
 * else -1 / 0. */
int pg_gvcf_ref_table(const char *ref_names, const int64_t *name_off, int32_t n_seq, int32_t *table, uint32_t mask);
int pg_gvcf_text(const pg_gvcf_cfg *cfg, const int32_t *sel_col, const int32_t *prev_same, const char *ref_names, const int64_t *name_off,
                 const int64_t *seq_len, const int64_t *seq_off, const int32_t *table, uint32_t mask, int32_t n_seq, const uint8_t *seq,
                 const char *text, int64_t len, int n_threads, char *out, int64_t out_cap, int64_t *rows_len_out, int64_t *n_rows_out,
                 int64_t *err_line_out, int *err_code_out);
/* Device route (csrc/pg_gvcf_dev.hip) for the regular spelling (fields split by single tabs, the header's field count, ASCII, a
 * position of digits only), the calls of the filter route's slot protocol (csrc/pg_line_slot.h):
 *   pg_gvcf_dev_config        the option set and the fasta, uploaded once; *taken_out = 0 when the device does not take the run (a
 *                             header too wide for the tab table in LDS, no output column), -1 when the sequences exceed the scratch
 *                             budget (PG_SCRATCH_GIB)
 *   pg_gvcf_dev_submit / _submit_bgzf / _set_output / _parse / _collect / _rows / _rows_bgzf / _text / _stats
 *                             as pg_filter_dev_*: k_gvcf_lines<0> sizes the rows, a scan places them, k_gvcf_lines<1> writes them
 *                             (and k_deflate makes them BGZF members); a line the device does not take hands the block to
 *                             pg_gvcf_text */
int pg_gvcf_dev_config(pg_ctx *ctx, const pg_gvcf_cfg *cfg, const int32_t *sel_col, const char *ref_names, const int64_t *name_off,
                       const int64_t *seq_len, const int64_t *seq_off, const int32_t *table, uint32_t mask, int32_t n_seq, const uint8_t *seq,
                       int64_t seq_bytes, int *taken_out);
int pg_gvcf_dev_submit(pg_ctx *ctx, int slot, const char *text, int64_t len);
int pg_gvcf_dev_submit_bgzf(pg_ctx *ctx, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                            const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                            int64_t text_len);
int pg_gvcf_dev_set_output(pg_ctx *ctx, int bgzf_members);
int pg_gvcf_dev_parse(pg_ctx *ctx, int slot);
int pg_gvcf_dev_collect(pg_ctx *ctx, int slot, int64_t *rows_len_out, int64_t *n_rows_out, int64_t *host_line_out, int64_t *bgzf_len_out,
                        int64_t *n_lines_out);
int pg_gvcf_dev_rows(pg_ctx *ctx, int slot, uint8_t *dst, int64_t len);
int pg_gvcf_dev_rows_bgzf(pg_ctx *ctx, int slot, uint8_t *dst, int64_t len);
int pg_gvcf_dev_text(pg_ctx *ctx, int slot, uint8_t *dst, int64_t len);
int pg_gvcf_dev_stats(pg_ctx *ctx, int64_t *blocks_out, int64_t *host_blocks_out);

/* ---- biallelic `.geno` sites written as EIGENSTRAT rows (the genoToEigenstrat.py drop-in, genomics_general_amd/genoeig.py) --------
 * Replaces the per-site loop of tools/genoToEigenstrat.py:48-73 with parseGenoLine (genomics.py:1884-1902), Genotype / asCount
 * (317-370) and GenomeSite.alleles / asList("count") (535-557).  The per-site and per-cell rules are csrc/pg_eig_core.h.  The option
 * set: */
typedef struct pg_eig_cfg {
    int32_t in_fmt;                                          /* -f 0 phased 1 diplo */
    int32_t n_sel;                                           /* written columns (-s; a header name given twice counts twice) */
    int32_t n_cols;                                          /* fields of the header line */
    int32_t universal_newlines;                              /* 1: a file read in text mode; 0: stdin, where \r is whitespace */
    int32_t cumulative;                                      /* --cumulativePos */
    int32_t n_scaf;                                          /* scaffolds of the --chromFile */
} pg_eig_cfg;
/* what one block hands the next */
typedef struct pg_eig_state {
    int64_t sites;                                           /* sites in front of the block (the .snp row's index) */
    int64_t pos;                                             /* --cumulativePos: the last written position */
    int64_t scaf_len;                                        /*   bytes of the last kept site's scaffold in scaf_io, -1: none yet */
    int32_t entry;                                           /*   its label's entry, -1: none yet */
    int32_t pad;
} pg_eig_state;
/* The tables beside them: sel_col[n_sel] the header field of each written column (a name the header holds twice: its last field),
 * prev_same / next_same[n_cols] the field before / behind with the same name or -1 (dict(zip(names, cells)): of a repeated name the
 * last cell the line has counts, once), both NULL for a header without repeats; the --chromFile as n_scaf scaffold names side by side
 * (names, name_off[n_scaf + 1]) under an open-addressed table (pg_gvcf_ref_table), their labels side by side (labels,
 * label_off[n_scaf + 2]: entry n_scaf is str(nullChrom), every other scaffold's label); with --cumulativePos label_key[n_scaf + 1]
 * the slot of each entry's label in offsets[] or -1 (the reference's KeyError), offsets[] the chromosomes' offsets and scaf_io the
 * last kept site's scaffold (room for max(len, state->scaf_len) bytes), all three carried from block to block with *state.
 *
 * Host route, every spelling line.split() takes: text[0 .. len) holds lines behind the header ('#' lines are no sites); the .geno
 * rows -> geno[0 .. geno_cap), the .snp rows -> snp[0 .. snp_cap) when both fit (then *state moves on), their bytes either way.  A
 * line on which the reference dies: *err_line_out its index in the block, *err_code_out the PGE_E_* code (pg_eig_core.h), the rows
 * before it written; else -1 / 0.  *n_sites_out: the sites walked. */
int pg_eig_text(const pg_eig_cfg *cfg, const int32_t *sel_col, const int32_t *prev_same, const int32_t *next_same, const char *names,
                const int64_t *name_off, const int32_t *table, uint32_t mask, const char *labels, const int64_t *label_off,
                const int32_t *label_key, pg_eig_state *state, int64_t *offsets, char *scaf_io, const char *text, int64_t len, int n_threads,
                char *geno, int64_t geno_cap, char *snp, int64_t snp_cap, int64_t *geno_len_out, int64_t *snp_len_out, int64_t *n_rows_out,
                int64_t *n_sites_out, int64_t *err_line_out, int *err_code_out);
/* Device route (csrc/pg_eig_dev.hip) for the regular spelling (fields split by single tabs, the header's field count, ASCII, a
 * position of digits only, cells of at most nine alleles), the calls of the slot protocol (csrc/pg_line_slot.h):
 *   pg_eig_dev_config         the option set and the --chromFile, uploaded once; *taken_out = 0 when the device does not take the run
 *                             (--cumulativePos, a header too wide for the tab table in LDS, no written column), -1 when the
 *                             --chromFile exceeds PG_EIG_MAX_SCAF scaffolds or PG_EIG_MAX_LABEL bytes in a label
 *   pg_eig_dev_submit / _submit_bgzf / _collect / _text / _stats   as pg_gvcf_dev_*
 *   pg_eig_dev_parse          first_site: the sites in front of the block; k_eig_lines<0> counts over all columns, decides, sizes
 *                             the .snp rows, k_rows_scan ranks and places them, k_eig_lines<1> writes both outputs; *n_lines_out the
 *                             block's lines
 *   pg_eig_dev_rows           which = 0 the .geno rows (n_rows (n_sel + 1) bytes), 1 the .snp rows */
#define PG_EIG_MAX_SCAF (1 << 22)
#define PG_EIG_MAX_LABEL 255
int pg_eig_dev_config(pg_ctx *ctx, const pg_eig_cfg *cfg, const int32_t *sel_col, const char *names, const int64_t *name_off,
                      const int32_t *table, uint32_t mask, const char *labels, const int64_t *label_off, int *taken_out);
int pg_eig_dev_submit(pg_ctx *ctx, int slot, const char *text, int64_t len);
int pg_eig_dev_submit_bgzf(pg_ctx *ctx, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                           const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                           int64_t text_len);
int pg_eig_dev_parse(pg_ctx *ctx, int slot, int64_t first_site, int64_t *n_lines_out);
int pg_eig_dev_collect(pg_ctx *ctx, int slot, int64_t *snp_len_out, int64_t *n_rows_out, int64_t *host_line_out, int64_t *n_lines_out);
int pg_eig_dev_rows(pg_ctx *ctx, int slot, int which, uint8_t *dst, int64_t len);
int pg_eig_dev_text(pg_ctx *ctx, int slot, uint8_t *dst, int64_t len);
int pg_eig_dev_stats(pg_ctx *ctx, int64_t *blocks_out, int64_t *host_blocks_out);

/* ---- `.geno` sites written as PED rows and MAP lines (the genoToPlink.py drop-in, genomics_general_amd/genoplink.py) --------------
 * Replaces tools/genoToPlink.py:36-72 -- nonOverlappingSitesWindows(windSites=inf) (genomics.py:2176-2223), seqDict (1790-1793),
 * splitSeq (390-396) and the interleaving of its zips -- with a byte transpose in which a cell expands into its alleles, each
 * followed by a blank.  The per-cell rules are csrc/pg_ped_core.h.  The option set: */
typedef struct pg_ped_cfg {
    int32_t fmt;                                             /* -f 0 phased 1 diplo 2 haplo / pairs / alleles (every character an allele) */
    int32_t n_sel;                                           /* rows of the .ped (-s, or every sample of the header) */
    int32_t n_cols;                                          /* fields of the header line */
    int32_t exact_cols;                                      /* no -s: a line must hold exactly the header's cells (addSite asserts) */
} pg_ped_cfg;
/* What the host route makes of a block (free with pg_ped_free).  A run is a stretch of sites of one scaffold (a scaffold that comes
 * back opens a new one; the block's first site always opens one: the driver joins it to the block before).  Sample q's bytes lie at
 * seq[seq_off[q] .. seq_off[q + 1]): run after run, site after site, the site's alleles each followed by a blank -- as many alleles
 * as the SHORTEST cell of that sample in that run of the block gives (run_min[r * n_sel + q] its length: zip() cuts every cell to it). */
typedef struct pg_ped_block {
    int64_t n_sites, n_runs, seq_bytes, map_bytes;
    uint8_t *seq;
    int64_t *seq_off;                                        /* n_sel + 1 */
    int64_t *run_start;                                      /* n_runs: the run's first site in the block */
    int64_t *run_name;                                       /* 2 n_runs: where the scaffold's name lies in the text, its length */
    int32_t *run_min;                                        /* n_runs x n_sel */
    uint8_t *map;                                            /* the .map rows: scaffold ' ' position " 0 " position '\n' */
    int64_t err_line;                                        /* the line the run stops on (-1: none) ... */
    int32_t err_code;                                        /* ... and why (PGP_E_*, pg_ped_core.h) */
} pg_ped_block;
/* Host route, every spelling line.split() takes, cells of any length: text[0 .. len) holds lines ended by \n behind the header ('#'
 * lines are no sites); sel_col[n_sel] the header field of each row's sample. */
int pg_ped_text(const pg_ped_cfg *cfg, const int32_t *sel_col, const char *text, int64_t len, int n_threads, pg_ped_block *out);
void pg_ped_free(pg_ped_block *blk);
/* Device route (csrc/pg_ped_dev.hip) for the regular spelling (fields split by single tabs, the header's field count, ASCII, a
 * position of digits only) and cells of the configured lengths, the calls of the slot protocol (csrc/pg_line_slot.h):
 *   pg_ped_dev_config         the option set and sel_len[n_sel], the length every cell of a sample must have (the file's first site
 *                             sets it); tile_seqs: samples per tile of k_ped_tile (0: as many as the LDS holds); *taken_out = 0 when
 *                             the device does not take the run (a cell of more than PG_PED_DEV_ALLELES alleles or of an even length
 *                             under phased, a header too wide for the tab tables in LDS)
 *   pg_ped_dev_submit / _submit_bgzf / _stats   as pg_eig_dev_*; pg_ped_dev_text as pg_seq_dev_text
 *   pg_ped_dev_parse          k_ped_lines checks the lines and sizes the .map rows, two scans place the sites and the rows,
 *                             k_ped_map writes the rows, k_ped_tile transposes
 *   pg_ped_dev_collect        waits.  *host_line_out < 0: *n_sites_out sites, *map_len_out bytes of .map rows, the samples' bytes in
 *                             a matrix of pitch *pitch_out sites: sample q's 2 a_q bytes a site begin at 2 (a_0 + .. + a_(q-1)) x
 *                             pitch (pg_ped_dev_rows: which = 0 the first len bytes of the matrix, 1 the .map rows); else the block
 *                             goes to pg_ped_text
 *   pg_ped_dev_meta           per site of the collected block: 1 where it opens a run, where its line begins in the text */
#define PG_PED_DEV_ALLELES 4
int pg_ped_dev_config(pg_ctx *ctx, const pg_ped_cfg *cfg, const int32_t *sel_col, const int32_t *sel_len, int tile_seqs, int *taken_out);
int pg_ped_dev_submit(pg_ctx *ctx, int slot, const char *text, int64_t len);
int pg_ped_dev_submit_bgzf(pg_ctx *ctx, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                           const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                           int64_t text_len);
int pg_ped_dev_parse(pg_ctx *ctx, int slot);
int pg_ped_dev_collect(pg_ctx *ctx, int slot, int64_t *n_sites_out, int64_t *map_len_out, int64_t *host_line_out, int64_t *n_lines_out,
                       int64_t *pitch_out);
int pg_ped_dev_rows(pg_ctx *ctx, int slot, int which, uint8_t *dst, int64_t len);
int pg_ped_dev_meta(pg_ctx *ctx, int slot, uint8_t *run_dst, int64_t *start_dst);
int pg_ped_dev_text(pg_ctx *ctx, int slot, int64_t off, int64_t len, uint8_t *dst);
int pg_ped_dev_tile_seqs(pg_ctx *ctx, int *tile_seqs_out);
int pg_ped_dev_stats(pg_ctx *ctx, int64_t *blocks_out, int64_t *host_blocks_out);

/* ---- `.geno` lines turned into sequences (the genoToSeq.py drop-in, genomics_general_amd/genoseq.py) -----------------------------
 * Replaces the per-site loop of genoToSeq.py: parseGenoLine (genomics.py:1884-1902), GenoWindow.addSite / seqDict (1753-1793) and the
 * join of makeAlnString (2232-2251) -- a byte transpose, site-major text in, sequence-major bytes out.  The per-line and per-cell rules
 * are csrc/pg_seq_core.h.  The option set: */
typedef struct pg_seq_cfg {
    int32_t n_cols;                                          /* fields of the header line */
    int32_t n_seq;                                           /* output sequences */
    int32_t split;                                           /* --splitPhased: a sequence is one character of a cell */
    int32_t n_to_gap;                                        /* --NtoGap */
    int32_t exact_cols;                                      /* every column is taken (no -S): a line with more fields than the header
                                                                stops the run too */
} pg_seq_cfg;
/* The tables beside it, one entry per output sequence: sel_col the file column (2 ..), sel_off the character's offset within the cell
 * (0 when the cell is copied whole), sel_len the length the cell must have (2 * ploidy - 1 under --splitPhased; 0: any, copied whole).
 *
 * What a block of lines gives: */
typedef struct pg_seq_block {
    int64_t n_sites, n_runs;
    int64_t stride;                                          /* > 0: every sequence has `stride` bytes per site, sequence q lies at
                                                                seq + q * n_sites * stride; 0: see off */
    int64_t seq_bytes;
    uint8_t *seq;                                            /* the sequences' bytes, one sequence after the other */
    int64_t *off;                                            /* stride == 0: [n_seq][n_sites + 1] places in seq (site i of sequence q:
                                                                off[q * (n_sites + 1) + i] up to the entry behind it) */
    int64_t *pos;                                            /* [n_sites] */
    int64_t *run_start;                                      /* [n_runs] first site of every scaffold run of the block */
    int64_t *run_name;                                       /* [n_runs][2] where the run's scaffold stands in text: offset, length */
    int64_t err_line;                                        /* -1, or the block's line (0-based, '#' lines counted) the reference dies on; */
    int32_t err_code;                                        /*   why: PGS_E_* (pg_seq_core.h).  The sites in front of it are complete */
} pg_seq_block;
/* Host route, every spelling line.split() takes: text[0 .. len) holds whole lines (the last may lack its line feed), lines that begin
 * with '#' are skipped.  Free the block's arrays with pg_seq_free. */
int pg_seq_text(const pg_seq_cfg *cfg, const int32_t *sel_col, const int32_t *sel_off, const int32_t *sel_len, const char *text, int64_t len,
                pg_seq_block *out);
void pg_seq_free(pg_seq_block *block);
/* Device route (csrc/pg_seq_dev.hip) for the regular spelling (fields split by single tabs, the header's field count, ASCII, selected
 * cells of 2 * ploidy - 1 characters under --splitPhased and of one character otherwise), two slots in flight:
 *   pg_seq_dev_config       the option set; tile_seqs: output sequences per tile of k_seq_tile (0: as many as the LDS holds);
 *                           *taken_out = 0 when the device does not take it (a header too wide for the tab tables in LDS)
 *   pg_seq_dev_submit       a block of whole lines -> the tokenizer's text slot `slot` (0 / 1), its line feeds listed there
 *   pg_seq_dev_submit_bgzf  the same for a block still deflated (bgzip's members, pg_bgzf_walk's table; head: text in front of them):
 *                           the members cross PCIe deflated and k_inflate writes their text into the slot
 *   pg_seq_dev_parse        queues k_seq_lines, the scan of the kept lines, k_seq_rows and k_seq_tile
 *   pg_seq_dev_collect      waits.  *host_line_out < 0: the matrix [n_seq][*n_sites_out] is ready for pg_seq_dev_rows, the sites'
 *                           positions, run flags (1: the scaffold differs from the site before; the block's first site always) and
 *                           line starts for pg_seq_dev_meta; else line *host_line_out of the block is one the device does not take: the
 *                           block goes to pg_seq_text (pg_seq_dev_text brings its text back).  *n_lines_out: the block's line feeds,
 *                           *pitch_out: bytes between two sequences of the matrix on the device
 *   pg_seq_dev_rows         sequences q0 .. q1 - 1 of the matrix, `width` bytes of each (up to the pitch), -> dst with dst_pitch bytes
 *                           between them (page-locked memory makes it one DMA)
 *   pg_seq_dev_meta         pos_dst[n_sites], run_dst[n_sites], start_dst[n_sites] (where each site's line begins in the text)
 *   pg_seq_dev_text         len bytes of the collected block's text from offset off
 *   pg_seq_dev_stats        blocks transposed on the device / handed to the host so far; milliseconds of k_seq_lines and of k_seq_tile
 *                           (HIP events, only under pg_seq_dev_timing(ctx, 1): the events make collect wait for each kernel) */
int pg_seq_dev_config(pg_ctx *ctx, const pg_seq_cfg *cfg, const int32_t *sel_col, const int32_t *sel_off, const int32_t *sel_len,
                      int tile_seqs, int *taken_out);
int pg_seq_dev_submit(pg_ctx *ctx, int slot, const char *text, int64_t len);
int pg_seq_dev_submit_bgzf(pg_ctx *ctx, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                           const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                           int64_t text_len);
int pg_seq_dev_parse(pg_ctx *ctx, int slot);
int pg_seq_dev_collect(pg_ctx *ctx, int slot, int64_t *n_sites_out, int64_t *host_line_out, int64_t *n_lines_out, int64_t *pitch_out);
int pg_seq_dev_rows(pg_ctx *ctx, int slot, int q0, int q1, uint8_t *dst, int64_t dst_pitch, int64_t width);
int pg_seq_dev_meta(pg_ctx *ctx, int slot, int64_t *pos_dst, uint8_t *run_dst, int64_t *start_dst);
int pg_seq_dev_text(pg_ctx *ctx, int slot, int64_t off, int64_t len, uint8_t *dst);
int pg_seq_dev_timing(pg_ctx *ctx, int on);
int pg_seq_dev_stats(pg_ctx *ctx, int64_t *blocks_out, int64_t *host_blocks_out, double *lines_ms_out, double *tile_ms_out);

/* ---- `.geno` files joined by site (the mergeGeno.py drop-in, genomics_general_amd/mergegeno.py) ------------------------------------
 * Replaces the walk of mergeGeno.py:57-88 over every position of every scaffold of the .fai: a sorted join of text files.  A site is
 * (line of the scaffold in the .fai, position); a file gives the longest prefix of its lines whose sites are valid and increasing
 * (the first other line stops it).  The per-line rules are csrc/pg_merge_core.h, the planning of the rounds csrc/pg_merge_plan.h.
 * The option set: */
typedef struct pg_merge_cfg {
    int32_t n_files;                                         /* 1 .. 32 */
    int32_t method;                                          /* 0 intersect, 1 union, 2 all */
    int32_t union_min;                                       /* max(--unionMin, --mustIncludeFirst) */
    int32_t must_first;                                      /* --mustIncludeFirst */
    uint32_t out_mask;                                       /* bit f: the cells of file f are written (--outputOnly) */
    int32_t sep_len, missing_len;                            /* bytes of --outSep and of --missing */
    int32_t n_fai;                                           /* scaffolds of the .fai */
} pg_merge_cfg;
/* The .fai beside it: the names side by side in fai_names, name f at name_off[f] .. name_off[f + 1], and the lengths.
 *
 * One input file of a round of the host route: */
typedef struct pg_merge_input {
    const char *text;                                        /* its resident lines (whole lines; the last may lack its line feed when */
    int64_t len;                                             /*   nothing follows) */
    int32_t open;                                            /* 1: the input goes on behind them */
    int32_t n_cols;                                          /* fields of its header */
    int32_t prev_scaf;                                       /* in: the key of the last line the rounds before consumed (scaffold -1: */
    int64_t prev_pos;                                        /*   none); out: of the last line consumed so far */
    int32_t stop;                                            /* out: PGM_STOP_* when a line of this block stops the file */
    int64_t stop_line;                                       /*   that line (0-based in the block) */
    int64_t lines_done, bytes_done;                          /* out: lines and bytes of the block at or below the horizon */
} pg_merge_input;
typedef struct pg_merge_result {
    char *out;                                               /* the written lines */
    int64_t out_len, rows;
    int32_t from_scaf, hor_scaf;                             /* in: the horizon of the round before ({0, 0} at the start); out: this */
    int64_t from_pos, hor_pos;                               /*   round's horizon */
    int32_t last;                                            /* nothing is left behind this round */
    int32_t stalled;                                         /* an open file held no consumable line: nothing was written, read it further */
    int32_t err_code, err_file;                              /* PGM_E_* (pg_merge_core.h): the input is rejected; which file, */
    int64_t err_line;                                        /*   which line of its block */
} pg_merge_result;
/* Host route, every spelling line.split() takes: one round over the files' resident lines (its horizon planned by pg_merge_plan.h from
 * the keys found here; out_cap: the output budget of a round of the methods that write sites no file holds -- bytes of
 * lines no file adds to; the resident input does not come off it).  Free res->out with pg_merge_free. */
int pg_merge_text(const pg_merge_cfg *cfg, const char *sep, const char *missing, const char *fai_names, const int64_t *name_off,
                  const int64_t *fai_len, pg_merge_input *files, int64_t out_cap, pg_merge_result *res);
void pg_merge_free(pg_merge_result *res);
/* The plan of a round of the device route (pg_merge_plan.h), from pg_merge_dev_keys' info and from whether each file's input goes on.
 * round: [0] [1] where the round begins, [2] [3] its horizon, [4] stalled, [5] last, [6] the candidates are positions (dense) */
int pg_merge_plan(const pg_merge_cfg *cfg, const int64_t *fai_len, const int32_t *n_cols, int64_t max_name, const int64_t *info,
                  const int32_t *open, int64_t out_cap, int32_t from_scaf, int64_t from_pos, int64_t *round);
/* Device route (csrc/pg_merge_dev.hip) for the regular spelling (fields split by single tabs, no other ASCII whitespace, the header's
 * field count, ASCII, a final line feed) and a one-byte separator.  Every file owns a text region on the device; a round:
 *   pg_merge_dev_config       the option set, the .fai, per file the fields of its header; *taken_out = 0 when the device does not
 *                             take it (a separator that is not one byte, --missing beyond 64 bytes, a header of fewer than two fields)
 *   pg_merge_dev_submit       a block of whole lines of file f, behind the lines the rounds before left in its region
 *   pg_merge_dev_submit_bgzf  the same for a block still deflated (bgzip's members, pg_bgzf_walk's table; head: text in front of
 *                             them): k_inflate writes the text, with its line feeds listed
 *   pg_merge_dev_keys         k_merge_keys over the new lines and the scan for the stopping line.  Per file, info[f * 8 ..]: [0] lines
 *                             resident, [1] consumable lines among them, [2] the last one's scaffold, [3] its position, [4] PGM_STOP_*
 *                             when a line stops the file, [5] that line (counted in the region), [6] 1: a line outside the regular
 *                             spelling at or in front of it (the round is pg_merge_text's), [7] bytes resident (what the rounds consumed not counted)
 *   pg_merge_dev_merge        the round behind (from_scaf, from_pos) up to the horizon: k_merge_lines or k_merge_pos, the scan of the lines' lengths,
 *                             k_merge_emit, and -- pg_merge_dev_set_output(ctx, 1) -- k_deflate over the lines.  dense: the candidates
 *                             are the positions of the range (one scaffold), else the lines of the files.  done[f * 4 ..]: lines and
 *                             bytes of file f the round consumed, the key of its last line consumed so far; *bytes_out, *rows_out, *bgzf_out: what pg_merge_dev_rows brings
 *   pg_merge_dev_rows         the written lines (bgzf = 0) or their BGZF members (bgzf = 1)
 *   pg_merge_dev_advance      after a round of the host route: the lines and bytes it consumed per file (done[f * 2 ..]), the keys it ended on
 *   pg_merge_dev_text         the resident text of file f (for pg_merge_text; a deflated block's text never was on the host)
 *   pg_merge_dev_stats        rounds merged on the device; milliseconds of k_merge_keys, of k_merge_lines / k_merge_pos and of k_merge_emit (HIP events,
 *                             only under pg_merge_dev_timing(ctx, 1)) */
int pg_merge_dev_config(pg_ctx *ctx, const pg_merge_cfg *cfg, const char *sep, const char *missing, const char *fai_names,
                        const int64_t *name_off, const int64_t *fai_len, const int32_t *n_cols, int *taken_out);
int pg_merge_dev_submit(pg_ctx *ctx, int f, const char *text, int64_t len);
int pg_merge_dev_submit_bgzf(pg_ctx *ctx, int f, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                             const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                             int64_t text_len);
int pg_merge_dev_keys(pg_ctx *ctx, int64_t *info);
int pg_merge_dev_set_output(pg_ctx *ctx, int bgzf);
int pg_merge_dev_merge(pg_ctx *ctx, int dense, int32_t from_scaf, int64_t from_pos, int32_t hor_scaf, int64_t hor_pos, int64_t *done,
                       int64_t *bytes_out, int64_t *rows_out, int64_t *bgzf_out);
int pg_merge_dev_rows(pg_ctx *ctx, int bgzf, uint8_t *dst, int64_t len);
int pg_merge_dev_advance(pg_ctx *ctx, const int64_t *done, const int32_t *prev_scaf, const int64_t *prev_pos);
int pg_merge_dev_text(pg_ctx *ctx, int f, uint8_t *dst, int64_t len);
int pg_merge_dev_timing(pg_ctx *ctx, int on);
int pg_merge_dev_stats(pg_ctx *ctx, int64_t *rounds_out, double *keys_ms_out, double *match_ms_out, double *emit_ms_out);
int pg_merge_dev_end(pg_ctx *ctx);

/* ---- sequences written as `.geno` sites (the seqToGeno.py drop-in, genomics_general_amd/seqgeno.py) --------------------------------
 * Replaces seqToGeno.py:38-98 -- parseFasta (genomics.py:2256-2261), haploToPhased (412-446) and the per-site joins -- with two
 * stages that meet in a residue store: the sequences' characters side by side, feeds and blanks gone.  The per-byte and per-line
 * rules are csrc/pg_s2g_core.h.  A line of the output is name '\t' str(x + 1) '\t' and the bytes of a row template: per byte
 * -1 - literal ('\t', '|', '\n'), or the index h of a haplotype, whose residue at site x stands at store[hap_off[h] + x].
 * Host route: pg_s2g_strip copies text[0 .. len) without its line feeds and blanks to dst (room for len bytes) and returns the bytes
 * written; pg_s2g_text writes the lines x0 .. x1 - 1 of a segment to out and returns out_len, which must be what the closed form
 * gives (pgs_line_start), else -1. */
int64_t pg_s2g_strip(const char *text, int64_t len, uint8_t *dst, int n_threads);
int64_t pg_s2g_text(const uint8_t *store, const char *name, int32_t name_len, const int64_t *hap_off, const int32_t *tmpl, int32_t tmpl_len,
                    int64_t x0, int64_t x1, uint8_t *out, int64_t out_len, int n_threads);
/* Device route (csrc/pg_s2g_dev.hip); the store lives on the device:
 *   pg_s2g_dev_begin          the store, with room for store_hint residues to begin with (it grows)
 *   pg_s2g_dev_submit / _submit_bgzf   a fasta block of whole lines into text slot `slot` (csrc/pg_line_slot.h), as pg_ped_dev_*
 *   pg_s2g_dev_parse          k_s2g_lines marks head lines, flags irregular bytes and counts residues, two scans rank the head lines
 *                             and place the lines, k_s2g_heads writes the head lines' records, k_s2g_gather copies the sequence
 *                             lines to store[base ..); open: a record is open where the block begins
 *   pg_s2g_dev_collect        waits.  *host_line_out < 0: *n_res_out residues stand behind base, *n_heads_out head lines were seen
 *                             (pg_s2g_dev_heads: three words each -- where the line begins in the text, its bytes, the block's
 *                             residues in front of it); else the block goes to pg_s2g_strip and back by pg_s2g_dev_put
 *   pg_s2g_dev_text           bytes of the collected block's text; pg_s2g_dev_put / _get: residues to / from the store
 *   pg_s2g_dev_plan           the output's description: the template (every haplotype once, in rising order), n_segs segments with
 *                             their names, sites and, per segment and haplotype, the store offset; tile_seqs: haplotypes per tile of
 *                             k_s2g_tile (0: as many as the LDS holds)
 *   pg_s2g_dev_emit           a range of the output: piece k the lines x0[k] .. x1[k] - 1 of segment seg[k]; k_s2g_tile writes
 *                             them, bgzf != 0: k_deflate makes BGZF members of them (pg_s2g_dev_rows: which = 0 rows, 1 members) */
int pg_s2g_dev_begin(pg_ctx *ctx, int64_t store_hint);
int pg_s2g_dev_submit(pg_ctx *ctx, int slot, const char *text, int64_t len);
int pg_s2g_dev_submit_bgzf(pg_ctx *ctx, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                           const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                           int64_t text_len);
int pg_s2g_dev_parse(pg_ctx *ctx, int slot, int64_t base, int open);
int pg_s2g_dev_collect(pg_ctx *ctx, int slot, int64_t *n_res_out, int64_t *n_heads_out, int64_t *host_line_out, int64_t *n_lines_out);
int pg_s2g_dev_heads(pg_ctx *ctx, int slot, int64_t *dst, int64_t n_heads);
int pg_s2g_dev_text(pg_ctx *ctx, int slot, int64_t off, int64_t len, uint8_t *dst);
int pg_s2g_dev_put(pg_ctx *ctx, int64_t off, const uint8_t *src, int64_t len);
int pg_s2g_dev_get(pg_ctx *ctx, int64_t off, int64_t len, uint8_t *dst);
int pg_s2g_dev_plan(pg_ctx *ctx, const int32_t *tmpl, int32_t tmpl_len, int32_t n_haps, const char *names, const int64_t *name_off,
                    int64_t n_segs, const int64_t *seg_sites, const int64_t *hap_off, int64_t store_len, int tile_seqs, int *tile_seqs_out);
int pg_s2g_dev_emit(pg_ctx *ctx, const int32_t *seg, const int64_t *x0, const int64_t *x1, int64_t n_pieces, int64_t out_len, int bgzf,
                    int64_t *bgzf_len_out);
int pg_s2g_dev_rows(pg_ctx *ctx, int which, uint8_t *dst, int64_t len);
int pg_s2g_dev_stats(pg_ctx *ctx, int64_t *blocks_out, int64_t *host_blocks_out, int64_t *out_ranges_out);

#ifdef __cplusplus
}
#endif
#endif /* POPGEN_HIP_H */
