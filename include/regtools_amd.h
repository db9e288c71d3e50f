/* include/regtools_amd.h -- C ABI of libregtools_amd.so, the MI355X (gfx950) drop-in for the
 * `regtools junctions extract` hot path.
 *
 * The reference has no FFI layer; its seam is the public interface of class JunctionsExtractor
 * (/root/reference/src/junctions/junctions_extractor.h:183-247).  Each entry point below names the
 * reference interface it replaces.  Pure C: plain pointers and sizes, no C++ or torch types.
 * INTEGRATION.md shows the binding a regtools maintainer would add.
 *
 * Error model (replaces `throw std::runtime_error(msg)` caught in junctions_main.cc:51-57): every call
 * returns 0 on success; otherwise nonzero with the reference's own message text in `err`.
 * There is NO CPU fallback: without a HIP device (or if the gfx950 code object cannot be loaded)
 * rgx_ctx_create fails loudly with RGX_ERR_NO_DEVICE.
 */
#ifndef REGTOOLS_AMD_H
#define REGTOOLS_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RGX_OK             0
#define RGX_ERR_OPEN       1  /* "Unable to open BAM/SAM file.\n\n"                      junctions_extractor.cc:505 */
#define RGX_ERR_INDEX      2  /* "Unable to open BAM/SAM index. Make sure ...\n\n"       junctions_extractor.cc:510 */
#define RGX_ERR_REGION     3  /* "Unable to iterate to region within BAM.\n\n"           junctions_extractor.cc:521 */
#define RGX_ERR_NO_DEVICE  4  /* no usable HIP device / code object: the product never falls back to a CPU */
#define RGX_ERR_DEVICE     5  /* HIP runtime error */
#define RGX_ERR_FORMAT     6  /* malformed BGZF/BAM beyond what the reference tolerates silently */
#define RGX_ERR_ARG        7
#define RGX_ERR_FASTA      8  /* "Unable to extract FASTA sequence for position ...\n\n" junctions_extractor.cc:553 */
#define RGX_ERR_ABORT      9  /* the reference abort()s on this input (`junctions extract -s XS`, and `identify -s XS` in the first variant's window that reads it: an
                               * aux field of unknown type in front of the strand tag of a spliced read, sam.c:1233-1252 skip_aux; a VCF record whose FORMAT
                               * names a Flag, vcf.c:1638-1639); the tool then prints what htslib printed and calls abort() itself, a library caller gets this code */
#define RGX_ERR_EXIT      10  /* the reference's LIBRARY ends the process with exit(1) on this input, past the tool's own error handling (a VCF sample with more
                               * fields than FORMAT has keys, vcf.c:1610-1614): err is all it prints; the tool prints it and exits with 1 */

typedef struct rgx_ctx rgx_ctx;   /* one per process+device: HIP stream(s) and a reusable HBM workspace */

/* Parameters of one extraction.
 * Replaces the JunctionsExtractor constructors (junctions_extractor.h:185-205) and the option parser
 * (junctions_extractor.cc:42-122).  rgx_extract_params_default fills the default-ctor values. */
typedef struct {
    const char *region;        /* "." = whole file (h:196); "chr:beg-end" as sam_itr_querys parses it */
    int32_t     strandness;    /* 0 XS tag, 1 RF, 2 FR, 3 intron-motif (cc:71-84) */
    char        strand_tag[2]; /* "XS" (h:192) */
    uint32_t    min_anchor;    /* 8   (h:186)  -a */
    uint32_t    min_intron;    /* 70  (h:187)  -m */
    uint32_t    max_intron;    /* 500000 (h:188) -M */
    const char *fasta_path;    /* NULL = "NA"; required by strandness 3 (cc:105-110) */
    /* shard of the BGZF member list handled by this call (multi-GPU): members are cut into
     * n_shards contiguous ranges balanced by compressed bytes; records belong to the shard their first
     * byte is in.  0/1 = everything. */
    int32_t     shard;
    int32_t     n_shards;
    /* -b (cc:82-84): also count, per junction, the cell barcodes of its supporting reads (set_junction_barcode, cc:362-374).
     * Needs the whole file in one shard. */
    int32_t     barcodes;      /* 0 */
    char        barcode_tag[2];/* "CB" (h:192, h:204) */
} rgx_extract_params;

void rgx_extract_params_default(rgx_extract_params *p);

/* Result table, structure-of-arrays, rows in the reference's output order
 * (compare_junctions, junctions_extractor.h:117-140).  Replaces vector<Junction> from
 * JunctionsExtractor::get_all_junctions (cc:238-246); `left_ok && right_ok` is the filter
 * print_all_junctions applies (cc:267).  Owned by the library; release with rgx_table_free. */
typedef struct {
    int32_t    n_ref;
    char     **ref_name;        /* header->target_name */
    uint32_t  *ref_len;
    uint64_t   n;               /* rows */
    int32_t   *tid;
    uint32_t  *start, *end;     /* Junction::start/end (BED::start/end) */
    uint32_t  *thick_start, *thick_end;
    uint32_t  *read_count;
    uint64_t  *name_index;      /* k of "JUNC%08d" (get_new_junction_name, cc:152-157) */
    char      *strand;
    uint8_t   *left_ok, *right_ok;
    /* statistics (not part of the reference interface) */
    uint64_t   n_records;       /* alignments iterated in this shard */
    uint64_t   n_events;        /* junction events that passed junction_qc */
    uint64_t   inflated_bytes, compressed_bytes, n_members;
    double     ms_total, ms_inflate, ms_records, ms_scan, ms_reduce; /* wall + HIP-event stage times */
    /* partial (per-shard) tables also carry what a cross-shard merge needs */
    uint64_t  *first_seen;      /* event order of the first read of each row (shard-local) */
    uint64_t  *last_seen;       /* event order of the last read (its strand is the row's strand) */
    uint64_t   framing_sweeps;  /* statistics: verification sweeps of the speculative record framing (1 = every guess was right) */
    /* -b: Junction::barcodes (junctions_extractor.h:58) of every row, flattened.  Row i owns entries [bc_row_begin[i], bc_row_begin[i+1]),
     * listed in the order Junction::print_barcodes (h:99-111) writes them, i.e. the iteration order of the std::unordered_map the
     * reference keeps; entry k is the string bc_text[bc_str_begin[k] .. bc_str_begin[k+1]) seen bc_count[k] times.  All NULL unless
     * rgx_extract_params.barcodes was set. */
    uint64_t  *bc_row_begin;    /* n + 1 */
    uint32_t  *bc_count;
    uint64_t  *bc_str_begin;    /* entries + 1 */
    char      *bc_text;
    uint32_t  *bc_insert_rank;  /* entry k was the bc_insert_rank[k]-th distinct barcode its junction saw (0-based): a binding that refills a
                                 * Junction::barcodes inserts a row's entries in THIS order and the container iterates them in the listed order */
    double     ms_barcodes;     /* statistics: the barcode group-by (device + host ordering) */
    /* per-shard tables: nonzero when the record stream stopped inside this shard for a reason that ends iteration upstream (a member
     * that does not inflate, an empty member, an unreadable record) instead of reaching the shard's upper cut.  The merges ignore the
     * shards behind such a one: a later shard is a seek past the damage, a sequential reader never gets there. */
    uint64_t   stream_ended;
    double     ms_inflate_launch;   /* statistics: the whole-range DEFLATE launch alone, HIP events on the stream it ran on (0 = the range went up as several
                                     * launches).  Host input: the arrival-gated launch -- it spans the upload, its waves wait for their chunk; ms_inflate
                                     * is the pipeline stream's stage time, which with the early tail no longer covers that launch */
} rgx_junction_table;

int  rgx_ctx_create(int device, rgx_ctx **out, char *err, size_t errlen);
void rgx_ctx_destroy(rgx_ctx *ctx);
/* Statistics: the DEFLATE launch's time depends on where the arena's pages lie (12.8 / 13.9 / 15.0 ms for the same launch into ten arenas of one
 * process), so a context tries a few allocations on its first large call and keeps the fastest (REGTOOLS_AMD_ARENA=n, 0 = off; never in a one-shot
 * context).  ms[0] = the call's own arena, ms[1..] = the challengers; returns how many were timed by the last calibration (0 = none yet). */
int  rgx_ctx_arena_trials(const rgx_ctx *ctx, float *ms, int cap);

/* Replaces JunctionsExtractor::identify_junctions_from_BAM + get_all_junctions (cc:500-535, 238-246):
 * reads <bam_path> and its index (.csi before .bai, plain or BGZF-compressed: hts.c:2031-2042) from disk, uploads, runs the device pipeline, returns the table. */
int  rgx_extract(rgx_ctx *ctx, const char *bam_path, const rgx_extract_params *p,
                 rgx_junction_table **out, char *err, size_t errlen);

/* Same, input already in host memory (file bytes of the .bam and of its .bai or .csi) -- the configuration SURVEY.md 8(d) times:
 * "file bytes in host memory" -> "sorted junction table in host memory".  The file is uploaded in chunks on a copy stream while the
 * BGZF members of the chunks that have arrived are already being inflated; for that overlap the bytes should sit in page-locked memory
 * (rgx_host_alloc, or any hipHostMalloc / pinned allocation) -- pageable memory works, the copies then go through the driver's staging
 * buffer at a fraction of the link rate.  Replaces the file read of junctions_extractor.cc:503-525 (hts_open / sam_itr_querys). */
void *rgx_host_alloc(size_t bytes);      /* page-locked host memory (NULL when there is none to be had) */
void  rgx_host_free(void *p);
int  rgx_extract_mem(rgx_ctx *ctx, const void *bam, size_t bam_len, const void *bai, size_t bai_len,
                     const rgx_extract_params *p, rgx_junction_table **out, char *err, size_t errlen);

/* Several files in flight on one device (round 6).  Replaces the loop a cohort run makes around `regtools junctions extract` -- one process per BAM, one
 * after the other (junctions_main.cc:45-59).  A pipeline owns `depth` contexts on `device`; rgx_extract_submit hands file k to context k mod depth and
 * returns at once with a ticket, rgx_extract_wait returns that file's table (or its error) -- each file is one ordinary rgx_extract_mem call, so the
 * tables are those of sequential calls, while file k+1's upload and inflate run under file k's tail.  `bam` / `bai` must stay readable until the
 * file's rgx_extract_wait returns (page-locked memory: rgx_host_alloc); the parameter struct and its strings are copied by submit.  Tickets may be
 * waited for in any order, each once.  rgx_pipeline_destroy runs what is still queued to its end and frees tables nobody waited for.
 * Hardware queues: the HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES queues (4 unless the environment says otherwise WHEN HIP STARTS).
 * A pipeline works on four; with 16 or more the files' DEFLATE launches go out at once instead of in turns and a file costs ~7 % less;
 * depth > 2 is refused below 4 x depth. */
typedef struct rgx_pipeline rgx_pipeline;
int  rgx_pipeline_create(int device, int depth /* 1..8, 2 = one file's tail under the next one's upload */, rgx_pipeline **out, char *err, size_t errlen);
int  rgx_pipeline_depth(const rgx_pipeline *pl);
/* The context file `ticket` runs on.  After rgx_extract_wait its rows are still in that context's HBM (rgx_last_table_pack_device) until the file `depth`
 * tickets later is submitted: a rank of a multi-GPU job merges file k with the other ranks' there while file k+1 is already going up. */
rgx_ctx *rgx_pipeline_ctx(const rgx_pipeline *pl, uint64_t ticket);
int  rgx_extract_submit(rgx_pipeline *pl, const void *bam, size_t bam_len, const void *bai, size_t bai_len, const rgx_extract_params *p,
                        uint64_t *ticket, char *err, size_t errlen);
int  rgx_extract_wait(rgx_pipeline *pl, uint64_t ticket, rgx_junction_table **out, char *err, size_t errlen);
void rgx_pipeline_destroy(rgx_pipeline *pl);

/* Same, with the .bam bytes ALREADY RESIDENT IN HBM at d_bam (the measured configuration: bench.py, or a
 * pipeline that DMA'd the file straight to the device).  No host copy of the BAM is needed: even the BGZF
 * member chain (BSIZE at +16 of every member, bgzf.c:525) is discovered on the device.  Only the (small) .bai is
 * read on the host.  d_bam must be readable up to bam_len + 8 bytes. */
int  rgx_extract_device(rgx_ctx *ctx, const void *d_bam, size_t bam_len,
                        const void *bai, size_t bai_len, const rgx_extract_params *p,
                        rgx_junction_table **out, char *err, size_t errlen);

/* The same over several GPUs of one node from ONE host process: shard g of n_devices -- a contiguous BGZF member range
 * cut at record starts the index lists -- runs the whole pipeline on devices[g] from its own host thread; the shards' unique rows
 * (48 bytes each, packed in HBM on the shard's own stream) are gathered to devices[0] with ncclSend / ncclRecv in one group (RCCL over xGMI;
 * librccl.so.1 is loaded at run time; peer access is switched on per device pair) and merged there (rgx_table_merge_device).  Where RCCL cannot
 * be loaded, initialised or reports an error, the same rows travel as hipMemcpyPeerAsync copies and rgx_multi_exchange_kind() says so.  Shard order is file order: the table is the single-GPU table whatever n_devices is.  A device
 * may be listed more than once: those shards take turns on it and the exchange is a device copy (how a one-GPU box tests this path).
 * Replaces the call junctions_extract() makes into JunctionsExtractor (junctions_main.cc:45-59) on a multi-GPU node.  -b works across shards
 * (rgx_table_merge_barcodes).  The per-device contexts (workspace, streams) are created on first use and kept for the life of the process;
 * concurrent calls take turns. */
int  rgx_extract_multi(const int *devices, int n_devices, const char *bam_path, const rgx_extract_params *p,
                       rgx_junction_table **out, char *err, size_t errlen);
int  rgx_extract_multi_mem(const int *devices, int n_devices, const void *bam, size_t bam_len, const void *bai, size_t bai_len,
                           const rgx_extract_params *p, rgx_junction_table **out, char *err, size_t errlen);
/* How the last rgx_extract_multi* call of this process moved the shards' rows to the first device: "rccl grouped send/recv, N ranks, ...",
 * "hipMemcpyPeerAsync ... (RCCL not used: why)", "device copies (a device is listed more than once)", "none (one shard)".  The reference has
 * no counterpart (junctions_main.cc:45-59 is one process on one core); callers that report a multi-GPU run quote it (bench.py multi_gpu.exchange). */
const char *rgx_multi_exchange_kind(void);

void rgx_table_free(rgx_junction_table *t);

/* Merge per-shard tables (shard order = file order) into the final table: sum counts, min/max thick
 * bounds, earliest first_seen names the row, latest last_seen gives the strand; rows are renamed and
 * re-sorted.  This is the host-side half of the multi-GPU path; the device-side exchange is an
 * all-gather of the packed rows (see rgx_table_pack / rgx_table_unpack). */
int  rgx_table_merge(const rgx_junction_table *const *parts, int n_parts, uint32_t min_anchor,
                     rgx_junction_table **out, char *err, size_t errlen);

/* Fixed-width row packing for the RCCL all-gather: 48 bytes per row. */
#define RGX_PACKED_ROW_BYTES 48
size_t rgx_table_pack(const rgx_junction_table *t, void *dst, size_t dst_cap); /* returns bytes needed */
int    rgx_table_unpack(const void *src, size_t n_rows, const rgx_junction_table *names_from,
                        rgx_junction_table **out);
/* The barcode lists of a table as one byte block, and back onto a table of the same rows (rgx_table_unpack): what the ranks of the
 * one-process-per-GPU driver exchange next to the packed rows so that -b works there too (junctions_extractor.cc:204-217).  pack returns the bytes
 * needed (0 = no barcode lists) and writes when dst_cap suffices; unpack validates every offset. */
size_t rgx_table_pack_barcodes(const rgx_junction_table *t, void *dst, size_t dst_cap);
int    rgx_table_unpack_barcodes(rgx_junction_table *t, const void *src, size_t len);
/* -b across shards: fills merged->bc_* from the shards' tables (every one extracted with barcodes = 1; shard order = file order).  A junction's
 * barcodes are the shards' lists one after the other in first-seen order, equal strings summed, handed to the container the reference keeps
 * (junctions_extractor.cc:204-217, h:99-111).  rgx_table_merge and rgx_extract_multi call it themselves. */
int    rgx_table_merge_barcodes(const rgx_junction_table *const *parts, int n_parts, rgx_junction_table *merged, char *err, size_t errlen);
/* rgx_table_pack without the host: t must be the result of the LAST rgx_extract / rgx_extract_mem / rgx_extract_device call on this
 * context (its rows are then still in HBM; anything else is RGX_ERR_ARG and the caller packs on the host).  Writes t->n packed rows
 * to device memory at d_dst -- the all-gather input of the multi-GPU path. */
int    rgx_last_table_pack_device(rgx_ctx *ctx, const rgx_junction_table *t, void *d_dst, uint64_t cap_rows, char *err, size_t errlen);
/* The same merge with the gathered rows STILL IN HBM (what an RCCL all-gather leaves there): shard g's packed rows start at
 * d_rows + g * stride_rows * 48 bytes and there are part_rows[g] of them.  Sort, reduce, naming and output order run on the
 * device; one copy of the final rows comes back.  first_seen/last_seen of the result are the merge's own order words. */
int    rgx_table_merge_device(rgx_ctx *ctx, const void *d_rows, uint64_t stride_rows, const uint64_t *part_rows, int n_parts,
                              uint32_t min_anchor, const rgx_junction_table *names_from, rgx_junction_table **out,
                              char *err, size_t errlen);

/* Replaces Junction::print / print_all_junctions (junctions_extractor.h:90-98, cc:249-280): BED12 text.
 * only_anchored != 0 keeps rows with both anchors (the `junctions extract` output).  Returns the number
 * of bytes written, or the size needed when buf is NULL. */
size_t rgx_table_format_bed12(const rgx_junction_table *t, int only_anchored, char *buf, size_t cap);

/* Replaces Junction::print_barcodes as print_all_junctions calls it (h:99-111, cc:272-273): one line "<distinct>\t<bc>:<count>,...\n"
 * per printed row.  Same buffer protocol as rgx_table_format_bed12.  A table without barcodes gives "0\t\n" lines (what
 * `cis-splice-effects identify -b` writes: its extractor never collects any, identifier.cc:288, :239-241). */
size_t rgx_table_format_barcodes(const rgx_junction_table *t, int only_anchored, char *buf, size_t cap);

/* =====================================================================================================
 * Cohort matrix: the union of the junctions of many samples with one read-count column per sample.
 * Replaces the per-sample loop plus the merge a cohort run makes after junctions_main.cc:45-59 -- N BED files joined by a script; the reference has
 * no counterpart.  A cohort is an ordered list of samples (0..S-1 in the order added), each one junction table plus a name.
 *   rows that take part   only_anchored: the rows with both anchors, i.e. the lines of that sample's `junctions extract` BED12 (print_all_junctions,
 *                         junctions_extractor.cc:267), computed from the row's own numbers -- start - thick_start >= min_anchor && thick_end - end >=
 *                         min_anchor, unsigned 32-bit -- never from the flag bytes; otherwise every row
 *   contigs               matched by NAME: the cohort's list is the samples' header names in order of first appearance; one name with two lengths is
 *                         RGX_ERR_ARG (the message names the contig and both samples)
 *   key                   (cohort tid, start, end, strand class: '+' 0, '-' 1, anything else 2), the reference's own (junctions_extractor.cc:180-194);
 *                         a sample has at most one row per key
 *   per junction          n_with = samples that have it, total = sum of their read counts (64 bit), thick_start = min, thick_end = max, strand = the
 *                         character of the highest-numbered sample that has it; the per-sample counts as a CSR image
 *   order and names       rows ascend by (cohort tid, start, end, class); row i is JUNC%08d of i + 1 (the cohort's own rule)
 *   filters               rows below min_samples or min_total are dropped before naming
 * ===================================================================================================== */
typedef struct rgx_cohort rgx_cohort;
typedef struct { int32_t only_anchored; uint32_t min_samples; uint64_t min_total; } rgx_cohort_params;
/* Replaces nothing in the reference (see above): the finished matrix, structure-of-arrays, owned by the library (rgx_cohort_matrix_free). */
typedef struct {
    int32_t    n_ref;           /* the cohort's contig table */
    char     **ref_name;
    uint32_t  *ref_len;
    uint32_t   n_samples;
    char     **sample_name;
    uint64_t   n;               /* rows */
    uint32_t  *tid;             /* index into ref_name */
    uint32_t  *start, *end, *thick_start, *thick_end;
    char      *strand;
    uint32_t  *n_with;          /* samples that have the row */
    uint64_t  *total;           /* sum of their read counts */
    uint64_t  *row_begin;       /* n + 1: row i owns col_sample / val_count [row_begin[i], row_begin[i + 1]) */
    uint32_t  *col_sample;      /* ascending within a row */
    uint32_t  *val_count;
    /* statistics */
    double     ms_add_total;    /* host time spent inside the adds so far (device path: a scan of the host table and an enqueue) */
    double     ms_finish;       /* this finish, wall, up to the rows being in host memory */
    uint64_t   n_triples;       /* (junction, sample, count) triples accumulated */
} rgx_cohort_matrix;
void rgx_cohort_params_default(rgx_cohort_params *p);                       /* 1, 1, 1 */
/* The accumulator lives in the HBM of ctx's device (blocks of 4 M triples, 28 bytes each; blocks are added, never re-copied).  Fewer than 2^24 samples
 * and at most 2^32 - 2^16 triples (RGX_ERR_ARG beyond either); RGX_ERR_DEVICE when HBM runs out. */
int  rgx_cohort_create(rgx_ctx *ctx, const rgx_cohort_params *p, rgx_cohort **out, char *err, size_t errlen);
/* src_ctx: the context t came from (rgx_pipeline_ctx of the ticket for a pipeline's table), or NULL.  When t is still the last table of src_ctx on
 * the cohort's device the rows go device to device -- on the cohort's own stream, behind src_ctx's last kernel by an event, no host wait; src_ctx's
 * next call waits for that copy the same way, so add a pipeline's file k BEFORE submitting file k + depth.  Otherwise they are uploaded from t.  Same result. */
int  rgx_cohort_add(rgx_cohort *co, rgx_ctx *src_ctx, const rgx_junction_table *t, uint32_t min_anchor,
                    const char *sample_name, uint32_t *sample_index, char *err, size_t errlen);
int  rgx_cohort_add_path(rgx_cohort *co);   /* statistics: 1 = the last add took the device path, 0 = the upload */
/* One key-carrying radix sort of the triples, head flags, scans and single-writer segmented passes on the device; one copy of the matrix comes back.
 * May be called again after more adds. */
int  rgx_cohort_finish(rgx_cohort *co, rgx_cohort_matrix **out, char *err, size_t errlen);
void rgx_cohort_destroy(rgx_cohort *co);
void rgx_cohort_matrix_free(rgx_cohort_matrix *m);
/* Host twin of add + finish (as rgx_table_merge is of rgx_table_merge_device): plain C++ on host tables, its own code path, no device.  NOT a fallback:
 * it is what the device result is checked against.  min_anchor[k] and names[k] belong to tables[k]. */
int  rgx_cohort_merge_host(const rgx_junction_table *const *tables, const uint32_t *min_anchor, const char *const *names, int n,
                           const rgx_cohort_params *p, rgx_cohort_matrix **out, char *err, size_t errlen);
/* BED12 of the cohort, one line per row laid out as Junction::print does (junctions_extractor.h:90-98): chromStart/End and thickStart/End are the
 * cohort's thick bounds, the score is total, the blocks start - thick_start, thick_end - end and 0, end - thick_start.  Buffer protocol of
 * rgx_table_format_bed12. */
size_t rgx_cohort_format_bed12(const rgx_cohort_matrix *m, char *buf, size_t cap);
/* The counts table: "chrom\tstart\tend\tstrand" and one "\t<sample name>" per sample, then one line per row with the junction's own start / end and
 * S dense counts (0 where a sample lacks the key).  Same buffer protocol. */
size_t rgx_cohort_format_counts(const rgx_cohort_matrix *m, char *buf, size_t cap);

/* =====================================================================================================
 * Intron clusters of a cohort matrix: the junctions that hang together through shared splice sites, and per cluster and sample the reads
 * on it -- the denominators of the ratio "reads on this junction / reads on its cluster" that differential-splicing tools work with.
 * The reference has no counterpart; this is the cohort's own rule.  rgx_cohort_cluster is the FIRST step of LeafCutter-style clustering only:
 * there is NO re-clustering behind its filters -- a component is kept or dropped whole.  The refinement modelled on LeafCutter's (weak and
 * over-long introns leave, the rest is clustered again) is rgx_cohort_refine, further down.
 *   input                 any rgx_cohort_matrix m: from rgx_cohort_finish or rgx_cohort_merge_host, filtered or not
 *   graph                 rows i and j are linked when they have the same tid, the same strand class (m->strand[i]: '+' 0, '-' 1, anything
 *                         else 2) and the same start or the same end; a cluster is a connected component (transitive: A and B sharing a
 *                         start and B and C sharing an end puts all three in one)
 *   filters               a component is kept when it has at least min_rows rows and the sum of m->total over them is at least min_total;
 *                         the rows of a dropped one get cluster[i] = RGX_NO_CLUSTER
 *   numbering             kept clusters are 0 .. C-1, ascending by the index of their first (lowest) row in m
 *   denominators          per cluster, the samples whose counts over its rows sum to more than zero, ascending, and that sum (64 bit)
 *   limits                m->n and m->row_begin[m->n] each at most 2^32 - 2^16 (RGX_ERR_ARG beyond); RGX_ERR_DEVICE when workspace cannot be
 *                         had; an empty matrix gives n_clusters = 0 and cl_begin = cs_begin = [0]
 * ===================================================================================================== */
#define RGX_NO_CLUSTER 0xffffffffu
typedef struct { uint32_t min_rows; uint64_t min_total; } rgx_cluster_params;
/* Structure-of-arrays, owned by the library (rgx_cohort_clusters_free), one page-locked block like the matrix. */
typedef struct {
    uint64_t   n_rows;          /* = m->n */
    uint64_t   n_clusters;      /* C */
    uint32_t  *cluster;         /* n_rows: the row's cluster, or RGX_NO_CLUSTER */
    uint64_t  *cl_begin;        /* C + 1: cluster k owns cl_row [cl_begin[k], cl_begin[k + 1]) */
    uint32_t  *cl_row;          /* the member rows, ascending within a cluster */
    uint64_t  *cl_total;        /* C: sum of m->total over the members */
    uint64_t  *cs_begin;        /* C + 1: cluster k owns cs_sample / cs_total [cs_begin[k], cs_begin[k + 1]) */
    uint32_t  *cs_sample;       /* ascending within a cluster */
    uint64_t  *cs_total;        /* the cluster's reads in that sample (never 0) */
    /* statistics */
    uint32_t   n_rounds;        /* hook + jump rounds the component search ran, the one that changed nothing included (the twin: 0) */
    double     ms_cluster;      /* this call, wall, up to the result being in host memory */
    uint64_t   n_components;    /* before the filters */
    uint64_t   n_ineligible, n_weak;   /* rgx_cohort_refine: rows over max_intron, rows removed as weak (rgx_cohort_cluster: 0, 0) */
} rgx_cohort_clusters;
void rgx_cluster_params_default(rgx_cluster_params *p);                     /* 1, 0: everything is kept */
/* On the cohort's device and stream.  When m is the matrix of co's most recent finish its image is still in HBM and is read in place;
 * otherwise the columns needed (tid, start, end, strand, total, row_begin, col_sample, val_count) are uploaded.  Same result.  co may be a
 * cohort with no samples.  Two stable radix sorts of the rows give the edges (neighbours in a site group), hooking towards the smaller
 * label and pointer jumping give the components, and one key-carrying radix sort of the count entries gives the denominators. */
int  rgx_cohort_cluster(rgx_cohort *co, const rgx_cohort_matrix *m, const rgx_cluster_params *p, rgx_cohort_clusters **out,
                        char *err, size_t errlen);
int  rgx_cohort_cluster_path(rgx_cohort *co);   /* statistics: 1 = the last cluster call read the matrix in HBM, 0 = it uploaded it */
/* Host twin: sort-based site groups plus union-find in plain C++, its own code path, no device.  NOT a fallback: it is what the device result
 * is checked against. */
int  rgx_cohort_cluster_host(const rgx_cohort_matrix *m, const rgx_cluster_params *p, rgx_cohort_clusters **out, char *err, size_t errlen);
void rgx_cohort_clusters_free(rgx_cohort_clusters *cl);
/* The cluster counts in the layout of LeafCutter's perind.counts: "chrom" and one " <sample name>" per sample, then one line per clustered
 * row in matrix order: "<contig>:<start>:<end>:clu_<k>_<s>" (k = cluster + 1; s = +, - or NA by strand class) and one " <num>/<den>" per
 * sample -- the row's count in the sample over the cluster's, "0/0" where the sample has no reads in the cluster.  Rows with
 * RGX_NO_CLUSTER are left out.  Buffer protocol of rgx_cohort_format_counts. */
size_t rgx_cohort_format_cluster_counts(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, char *buf, size_t cap);

/* -----------------------------------------------------------------------------------------------------
 * Refined clusters, modelled on LeafCutter's refinement: introns that are too long never take part, junctions that are weak in their
 * cluster are removed, and what is left is clustered again, so one weak junction no longer ties strong clusters together and the
 * denominators are sums over the surviving rows only.  No claim of byte equality with LeafCutter: its ratio test is in floating point
 * (this one is exact) and its clusters start from overlapping introns (these from shared splice sites).  LeafCutter's customary settings
 * correspond to max_intron 100000, min_reads 5, ratio 1/1000, min_rows 2, min_total 30.
 *   eligible rows         max_intron == 0 || end - start <= max_intron; n_ineligible counts the others, which link nothing
 *   stage 1               the components of the eligible rows under the link rule above; T(i) = the sum of m->total over the eligible
 *                         rows of i's component
 *   weak rows             an eligible row is weak when total[i] < min_reads or total[i] * ratio_den < ratio_num * T(i) -- compared on the
 *                         whole products (up to 96 bits), equality passes; n_weak counts them
 *   stage 2               the components of the eligible rows that are not weak; one is kept when it has at least min_rows rows and its
 *                         summed total is at least min_total; kept clusters are numbered by their lowest row; ineligible rows, weak rows and
 *                         the rows of a dropped component get RGX_NO_CLUSTER; cl_* and cs_* are over member rows only; n_components counts
 *                         the stage-2 components; n_rounds is the sum of both searches' rounds
 *   one pass              removing rows and splitting components can only lower T, so a row that passed the ratio test passes it against
 *                         every later T, and min_reads does not depend on T: a second removal would remove nothing
 *   arguments             ratio_den == 0 or ratio_num > ratio_den is RGX_ERR_ARG; the limits are rgx_cohort_cluster's; an empty matrix gives
 *                         n_clusters = 0 without a launch
 * With the default parameters the result equals rgx_cohort_cluster's with the same min_rows / min_total in every array and count.  The
 * result is the same struct: the formatter above and rgx_cohort_clusters_free take it.  Both matrix paths apply (rgx_cohort_cluster_path).
 * ----------------------------------------------------------------------------------------------------- */
typedef struct { uint32_t max_intron;            /* rows with end - start > max_intron take no part; 0 = no limit */
                 uint64_t min_reads;             /* a row whose m->total is below this is weak */
                 uint32_t ratio_num, ratio_den;  /* a row is weak when total * ratio_den < ratio_num * T (T: its stage-1 component's total) */
                 uint32_t min_rows; uint64_t min_total;   /* the cluster filters of rgx_cluster_params, applied to the FINAL components */
} rgx_refine_params;
void rgx_refine_params_default(rgx_refine_params *p);   /* 0, 0, 0/1, 1, 0: nothing is removed */
int  rgx_cohort_refine(rgx_cohort *co, const rgx_cohort_matrix *m, const rgx_refine_params *p, rgx_cohort_clusters **out,
                       char *err, size_t errlen);
/* Host twin: union-find twice and unsigned __int128 for the ratio test, no device.  NOT a fallback. */
int  rgx_cohort_refine_host(const rgx_cohort_matrix *m, const rgx_refine_params *p, rgx_cohort_clusters **out, char *err, size_t errlen);

/* -----------------------------------------------------------------------------------------------------
 * The splicing phenotype table of a clustered cohort: per clustered junction and sample the intron-excision ratio, filtered, standardised
 * across samples and rank-normalised across junctions -- the table an sQTL mapper takes.  MODELLED ON LeafCutter's
 * prepare_phenotype_table.py, which is not available to this project: nothing here was compared against it, its means behind the
 * imputation are computed in another order, and its per-chromosome files are not written (its principal components: the next block).
 *   input                 a matrix m and a cluster result cl OF THAT MATRIX (rgx_cohort_cluster, rgx_cohort_refine or their twins);
 *                         cl->n_rows != m->n, or a cluster number at or above cl->n_clusters, is RGX_ERR_ARG.  S = m->n_samples
 *   parameters            na_num / na_den: the share of missing samples a row may have (na_den == 0 or na_num > na_den is RGX_ERR_ARG);
 *                         min_sd: the least deviation a row must show (negative or NaN is RGX_ERR_ARG).  Defaults 4 / 10 and 0.005
 *   candidates            the rows with cl->cluster[i] != RGX_NO_CLUSTER, n_clustered of them
 *   ratio                 for candidate row i of cluster c and sample s: num = the row's count in s, den = the cluster's cs_total in s,
 *                         either 0 where the CSR has no entry.  The entry is MISSING when den == 0; otherwise
 *                         x = ((double)num + 0.5) / ((double)den + 0.5)
 *   summation order       a sum over a row's present samples is 64 partials P[l], each starting at +0.0 and taking the present samples
 *                         with s % 64 == l in ascending s; then for off = 32, 16, 8, 4, 2, 1: P[l] = P[l] + P[l + off] for l < off; the
 *                         sum is P[0].  (A wave's strided loop and its __shfl_down halving.)  Part of the contract: mean and sd are
 *                         the same bits wherever they are computed
 *   row statistics        n_na = the missing samples; mean = sum(x) / (double)(S - n_na); sd = sqrt(sum(d * d) / (double)S), d = x - mean
 *                         over the present samples (a missing entry is imputed with the mean and adds nothing); d * d is a rounded
 *                         product, never fused into the add
 *   row filters           in this order: a row is dropped as missing when n_na == S or (uint64)n_na * na_den > (uint64)S * na_num
 *                         (n_drop_na); a row that stays is dropped as flat when !(sd > 0) or sd < min_sd (n_drop_sd); K rows are
 *                         kept, in matrix order
 *   standardised entry    z = (x - mean) / sd for a present entry, +0.0 for a missing one
 *   rank                  inside each sample's column over the K kept rows, z ascending, -0.0 equal to +0.0 (no NaN can occur):
 *                         rank2 = lo + hi, the 1-based first and last place of the entry's run of equal values -- twice its average
 *                         rank, an integer in [2, 2 K]
 *   quantile              rgx_pheno_quantile(rank2, K) = the standard normal quantile of rank2 / (2 (K + 1)), evaluated on the HOST by
 *                         Wichura's rational approximation AS 241 (PPND16): it needs log, which does not round alike on host and
 *                         device, and depends on (rank2, K) alone.  The result carries the integers; the text carries the quantiles
 *   limits                n_clustered * S at most 2^32 - 2^16 (RGX_ERR_ARG beyond, before any launch); RGX_ERR_DEVICE when workspace
 *                         cannot be had; no candidates, S == 0 or K == 0 give empty arrays
 * ----------------------------------------------------------------------------------------------------- */
typedef struct { uint32_t na_num, na_den;        /* a row is dropped when n_na * na_den > S * na_num */
                 double   min_sd;                /* ... or when its sd is below this (or not above 0) */
} rgx_pheno_params;
/* Structure-of-arrays, owned by the library (rgx_cohort_phenotypes_free), one block, page-locked on the device path. */
typedef struct {
    uint64_t   n_rows;          /* K */
    uint32_t   n_samples;       /* S */
    uint32_t  *row;             /* K: the kept rows of m, ascending */
    uint32_t  *n_na;            /* K: missing samples */
    double    *mean, *sd;       /* K */
    uint32_t  *rank2;           /* K * S, row-major: twice the average rank of the entry in its sample's column */
    /* statistics */
    uint64_t   n_clustered, n_drop_na, n_drop_sd;
    double     ms_pheno;        /* this call, wall, up to the result being in host memory */
} rgx_pheno_table;
void rgx_pheno_params_default(rgx_pheno_params *p);                         /* 4, 10, 0.005 */
/* On the cohort's device and stream; the matrix is found as rgx_cohort_cluster finds it (rgx_cohort_cluster_path reports which way).  A wave
 * per row for the statistics, a scan for the kept rows' places, one stable radix sort of the K * S entries by (sample, z), head flags and a scan
 * for the tie runs. */
int  rgx_cohort_phenotypes(rgx_cohort *co, const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_params *p,
                           rgx_pheno_table **out, char *err, size_t errlen);
/* Host twin: the same summation order in plain C++ and std::stable_sort per column, no device.  NOT a fallback. */
int  rgx_cohort_phenotypes_host(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_params *p,
                                rgx_pheno_table **out, char *err, size_t errlen);
void rgx_cohort_phenotypes_free(rgx_pheno_table *ph);
/* rank2 in [1, 2 K + 1]; anything else gives NaN. */
double rgx_pheno_quantile(uint32_t rank2, uint64_t n_rows);
/* "#Chr\tstart\tend\tID" and one "\t<sample name>" per sample, then one line per kept row: contig, start, end, the row's ID in
 * rgx_cohort_format_cluster_counts ("<contig>:<start>:<end>:clu_<k>_<s>") and per sample a tab and the quantile as %.17g.  ph must come from
 * (m, cl); 0 when the three do not fit together.  Buffer protocol of rgx_cohort_format_counts. */
size_t rgx_cohort_format_phenotypes(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph, char *buf,
                                    size_t cap);

/* -----------------------------------------------------------------------------------------------------
 * The principal components of the phenotype table: the covariates of an sQTL run, the .PCs file of LeafCutter's
 * prepare_phenotype_table.py (which calls sklearn's PCA on the quantile-normalised table; the tests compare with that library).
 *   input                 a phenotype table ph, of which only n_rows = K, n_samples = S and rank2 are read, and n_pcs
 *   errors                RGX_ERR_ARG, before any launch: K < 2 (or K > 2^31 - 1), S == 0, S > 2048, n_pcs == 0, n_pcs > min(K, S).
 *                         RGX_ERR_ARG also for a rank2 outside [2, 2 K]: the device notices it in its gather and reports it through a flag,
 *                         the twin when it meets it
 *   quantile table        T[r] = rgx_pheno_quantile(r, K) for r = 2 .. 2 K, computed on the HOST (2 K - 1 doubles, uploaded; log never runs
 *                         on the device); q[k][s] = T[rank2[k][s]]
 *   summation order       n_chunks = min(64, ceil(K / 1024)), L = ceil(K / n_chunks); chunk j is rows [j L, min(K, (j + 1) L)).  For
 *                         s <= t the chunk partial starts at +0.0 and takes acc = fma(q[k][s], q[k][t], acc) in ascending k;
 *                         gram[s][t] is the chunk partials added in ascending j from +0.0 by plain rounded adds, gram[t][s] = gram[s][t].
 *                         col_sum[s] likewise with acc = acc + q[k][s].  No floating-point atomics anywhere.  Part of the contract:
 *                         gram and col_sum are the same bits wherever they are computed
 *   covariance            on the host, by one function for the device path and the twin, contraction off:
 *                         cov[s][t] = (gram[s][t] - col_sum[s] * col_sum[t] / (double)K) / (double)(K - 1) for s <= t, mirrored
 *   eigen-decomposition   on the host, by that same function: cyclic Jacobi written here (no LAPACK).  variance = all S eigenvalues in
 *                         descending order; component = the first n_pcs unit eigenvectors, n_pcs x S row-major, each signed so that its
 *                         entry of largest absolute value (the first on ties) is positive -- sklearn 1.7's svd_flip(u_based_decision=False)
 *   limits                S <= 2048: the chunk partials are at most 64 S^2 doubles (2 GiB there) and the eigen-decomposition is O(S^3)
 *                         on one host thread.  RGX_ERR_DEVICE when workspace cannot be had
 * ----------------------------------------------------------------------------------------------------- */
/* Owned by the library (rgx_cohort_pheno_pcs_free), one block, page-locked on the device path. */
typedef struct {
    uint64_t   n_rows;          /* K */
    uint32_t   n_samples;       /* S */
    uint32_t   n_pcs;
    double    *col_sum;         /* S */
    double    *gram;            /* S * S, both triangles */
    double    *variance;        /* S: the eigenvalues of the covariance, descending */
    double    *component;       /* n_pcs * S, row-major */
    /* statistics, wall */
    double     ms_pcs;          /* this call */
    double     ms_gram;         /* behind the quantile table: the uploads, the kernels and the copy back (the twin: its Gram loops) */
    double     ms_eigen;        /* the host part: covariance, Jacobi, order and signs */
} rgx_pheno_pcs;
/* On the cohort's device and stream: rank2 and T are uploaded, k_pca_gram writes one partial per (pair of 64-sample tiles, chunk),
 * k_pca_reduce adds the chunks in order; one copy back and one host wait in front of the host part. */
int  rgx_cohort_pheno_pcs(rgx_cohort *co, const rgx_pheno_table *ph, uint32_t n_pcs, rgx_pheno_pcs **out, char *err, size_t errlen);
/* Host twin: the same order in plain C++ (std::fma), no device.  NOT a fallback. */
int  rgx_cohort_pheno_pcs_host(const rgx_pheno_table *ph, uint32_t n_pcs, rgx_pheno_pcs **out, char *err, size_t errlen);
void rgx_cohort_pheno_pcs_free(rgx_pheno_pcs *pcs);
/* "id" and one "\t<sample name>" per sample of m, then one line per component: its 1-based number and per sample a tab and the entry as
 * %.17g -- LeafCutter's .PCs layout.  pcs == NULL writes the header line alone; 0 when pcs is not of m's samples.  Buffer protocol of
 * rgx_cohort_format_counts. */
size_t rgx_cohort_format_pheno_pcs(const rgx_cohort_matrix *m, const rgx_pheno_pcs *pcs, char *buf, size_t cap);

/* -----------------------------------------------------------------------------------------------------
 * The nominal cis-sQTL scan of the phenotype table: for every table row and every variant within a window around its intron the regression of
 * the row's quantiles on the genotype dosage, with an intercept and the covariates in the model -- the nominal pass of FastQTL and tensorQTL,
 * neither of which is available to this project: the statistics are checked against ordinary least squares of the full model.
 *   input                 a phenotype table ph (n_rows = K, n_samples = S and rank2 are read); K regions, one per table row; V variants
 *                         {tid, pos}, pos 1-based, ascending by (tid, pos), equal keys allowed; their V x S int8 dosages, variant-major,
 *                         each 0, 1, 2 or -1 = missing; n_cov x S covariates, row-major (rgx_pheno_pcs.component), n_cov may be 0; window
 *   errors                RGX_ERR_ARG, before any launch: K == 0 or K > 2^31 - 1; V > 2^31 - 1; S > 2048; S < n_cov + 3 (the degrees of
 *                         freedom dof = S - n_cov - 2 are at least 1); variants out of order; a covariate that is, to rounding, a
 *                         combination of the intercept and the covariates before it.  RGX_ERR_ARG also for a dosage outside the four values
 *                         and for a rank2 outside [2, 2 K]: the device reports them through a flag word, the twin when it meets them
 *   basis                 on the HOST, by one function for the device path and the twin, contraction off: b_0 = all ones, b_j = covariate
 *                         j - 1; modified Gram-Schmidt over ascending j: v = b_j, then TWICE for i = 0 .. j - 1 in order d = sum_s v[s] q_i[s]
 *                         (plain rounded loop in ascending s from +0.0) and v[s] = v[s] - d * q_i[s] (rounded product, rounded difference);
 *                         |v| = sqrt(sum_s v[s] * v[s]); refused when !(|v| > 1e-10 * |b_j|); q_j[s] = v[s] / |v|.  C = n_cov + 1 vectors
 *   dot64(a, b)           64 partials P[l] from +0.0, each P[l] = fma(a[s], b[s], P[l]) for the s with s % 64 == l in ascending s; then for
 *                         off = 32, 16, 8, 4, 2, 1: P[l] = P[l] + P[l + off] for l < off; the result is P[0] (the phenotype table's order
 *                         with the product fused into the add)
 *   residual of x         for j = 0 .. C - 1 in order: d = dot64(x, q_j), then x[s] = fma(-d, q_j[s], x[s]) for every s; ss = dot64(x, x)
 *   phenotype row k       x[s] = T[rank2[k][s] - 2], T the quantile table of the principal components; residual Y[k], yy[k] = ss.  The row
 *                         is FLAT, and takes part in no pair, when !(yy > 1e-12 * S)
 *   variant v             n_present and the integer sum of the present dosages; verdict 1 (constant) when no sample is present or all
 *                         present dosages are equal -- an integer test, gg[v] = +0.0; else mean = (double)sum / (double)n_present, x[s] =
 *                         the dosage as a double, mean where it is missing; residual G[v], gg[v] = ss; verdict 2 (explained) when
 *                         !(gg > 1e-12 * S); verdict 0 (usable) otherwise
 *   pairs                 row k is cis to usable variant v when the tids are equal and start - min(start, window) <= pos <= end + window,
 *                         the right side saturating at 2^32 - 1.  A row's pairs are its cis variants in variant order: pair_begin[K + 1] and
 *                         pair_variant[P], an index into the input variants.  P > 2^32 - 2^16 is RGX_ERR_ARG
 *   per pair              dot = ONE chain acc = fma(Y[k][s], G[v][s], acc) in ascending s from +0.0; r = dot / sqrt(yy[k] * gg[v]);
 *                         slope = dot / gg[v]; every operation rounded on its own
 *   best                  best[k] = the pair of row k with the largest |r|, the earliest on ties; RGX_NO_PAIR for a row without pairs
 *   t and p               on the HOST (log never runs on the device): rgx_qtl_tstat and rgx_qtl_pvalue below
 *   limits                RGX_ERR_DEVICE when workspace cannot be had.  The device cuts the pairs into tiles of 64 rows x 64 usable variants;
 *                         more than 2^31 - 1 tiles (rows far out of position order at full size) is RGX_ERR_ARG
 * ----------------------------------------------------------------------------------------------------- */
#define RGX_NO_PAIR 0xffffffffu
typedef struct { uint32_t tid, start, end; } rgx_qtl_region;
/* Owned by the library (rgx_cohort_qtl_free), one block, page-locked on the device path. */
typedef struct {
    uint64_t   n_rows;          /* K */
    uint32_t   n_samples;       /* S */
    uint32_t   n_variants;      /* V */
    uint32_t   n_cov;
    uint32_t   dof;             /* S - n_cov - 2 */
    uint64_t   n_pairs;         /* P */
    uint8_t   *variant_verdict; /* V: 0 usable, 1 constant, 2 explained by the covariates */
    double    *yy;              /* K */
    double    *gg;              /* V */
    uint32_t  *pair_begin;      /* K + 1 */
    uint32_t  *pair_variant;    /* P */
    double    *r, *slope;       /* P */
    uint32_t  *best;            /* K: a pair, or RGX_NO_PAIR */
    /* statistics */
    uint64_t   n_constant, n_explained, n_flat_rows;
    uint64_t   n_tiles;         /* the device's tiles of 64 rows x 64 usable variants (the twin: 0) */
    double     ms_qtl;          /* this call, wall */
    double     ms_residual;     /* device time from the first upload to the sample-major residuals (the twin: its residual loops, wall) */
    double     ms_pairs;        /* device time of the pair products and the best pairs (the twin: its pair loops, wall) */
} rgx_qtl_result;
/* regions[k] = {m->tid, m->start, m->end}[ph->row[k]]; RGX_ERR_ARG when a row of ph is no row of m. */
int  rgx_cohort_pheno_regions(const rgx_cohort_matrix *m, const rgx_pheno_table *ph, rgx_qtl_region *out, char *err, size_t errlen);
/* On the cohort's device and stream: a wave per row and per variant for the residuals, a scan for the usable variants, a binary search per row
 * and two scans for the plan, ONE host wait for P, then one workgroup per (64 rows, 64 usable variants) and a wave per row for the best pair. */
int  rgx_cohort_qtl_nominal(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                            const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates,
                            uint32_t window, rgx_qtl_result **out, char *err, size_t errlen);
/* Host twin: the same chains in plain C++ (std::fma) and std::lower_bound, no device.  NOT a fallback. */
int  rgx_cohort_qtl_nominal_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                                 const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates, uint32_t window,
                                 rgx_qtl_result **out, char *err, size_t errlen);
void rgx_cohort_qtl_free(rgx_qtl_result *q);
/* t = r * sqrt(dof / (1 - r * r)); copysign(inf, r) when 1 - r * r <= 0. */
double rgx_qtl_tstat(double r, uint32_t dof);
/* The two-sided p of Student's t with dof degrees of freedom: the regularised incomplete beta I_x(dof / 2, 1 / 2) at x = dof / (dof + t * t)
 * by a Lentz continued fraction written here; 1 at t == 0, 0 for infinite t, NaN for NaN. */
double rgx_qtl_pvalue(double t, uint32_t dof);
/* "phenotype_id\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\tis_best" and one line per pair in CSR order: the row's ID of
 * rgx_cohort_format_phenotypes, variant_id[pair_variant], distance = (int64)var_pos - (int64)start of the row, r, slope, slope_se = slope /
 * tstat, tstat and the p-value as %.17g, is_best 1 or 0.  q must come from ph; q == NULL writes the header line alone; 0 when the arguments do
 * not fit together.  Buffer protocol of rgx_cohort_format_counts. */
size_t rgx_cohort_format_qtl(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph, const rgx_qtl_result *q,
                             const uint32_t *var_pos, const char *const *variant_id, char *buf, size_t cap);

/* -----------------------------------------------------------------------------------------------------
 * The permutation pass of the cis-sQTL scan: per table row the largest |r| over its cis variants, for the row as it is and for B permutations of
 * its samples, the empirical p of the row's best variant and its beta approximation -- FastQTL's --permute and tensorQTL's map_cis, neither of
 * which is available to this project: checked against a restatement in exact rationals, scipy and mpmath.  DELIBERATE DEVIATIONS: the degrees of
 * freedom are not re-estimated from the permutations, and the number of permutations is not adaptive.
 *   input                 everything rgx_cohort_qtl_nominal takes; n_perm = B; perm: (B + 1) x S uint16, row-major, row 0 the identity, every
 *                         row a permutation of 0 .. S - 1 (rgx_qtl_permutations fills one)
 *   errors                RGX_ERR_ARG, before any launch: the nominal scan's; B == 0 or B > 65535; row 0 not the identity; a row that is no
 *                         permutation; K (B + 1) > 2^32 - 2^16.  The flag words as in the nominal scan
 *   steps                 basis, dot64, residuals Y[k] with yy, G[v] with gg, verdicts, flat rows and cis ranges: the nominal contract's, unchanged.
 *                         No pair array is produced and P has no limit: n_cis[k] = the row's number of pairs, n_pairs their 64-bit sum
 *   per (k, b, cis v)     dot = ONE chain acc = fma(Y[k][perm[b][s]], G[v][s], acc) in ascending s from +0.0; r = dot / sqrt(yy[k] * gg[v]) with
 *                         the yy of the UNPERMUTED row, every operation rounded on its own
 *   perm_r[k][b]          the largest |r| over the row's cis variants, compared and stored as bit patterns (no order to fix), b = 0 .. B; +0.0
 *                         throughout for a row without pairs
 *   best                  of b = 0: best_variant[k] = the input variant with the largest |r|, the earliest on ties, RGX_NO_PAIR without pairs;
 *                         best_r[k] (signed) and best_slope[k] = dot / gg: bit for bit the nominal scan's r and slope at best[k]; +0.0 without
 *   n_ge, p_perm          n_ge[k] = #{b in 1 .. B: bits(perm_r[k][b]) >= bits(perm_r[k][0])}; p_perm[k] = (n_ge + 1) / (B + 1)
 *   beta approximation    on the HOST, by one function for the device path and the twin (rgx_qtl_beta_fit below), rows shared among threads,
 *                         each row's sums in ascending b: p_b = rgx_qtl_pvalue(rgx_qtl_tstat(perm_r[k][b], dof), dof) clipped to
 *                         [DBL_MIN, 1 - 2^-53] for b = 1 .. B; p_beta[k] = I_x(shape1, shape2) at x = rgx_qtl_pvalue(rgx_qtl_tstat(best_r[k],
 *                         dof), dof).  beta_status[k]: 0 converged, 1 the moment estimates kept, 2 no fit (no pairs, B < 2, zero variance or
 *                         moment estimates outside (0, inf)): shapes and p_beta NaN
 * ----------------------------------------------------------------------------------------------------- */
/* Owned by the library (rgx_cohort_qtl_perm_free), one block, page-locked on the device path. */
typedef struct {
    uint64_t   n_rows;          /* K */
    uint32_t   n_samples;       /* S */
    uint32_t   n_variants;      /* V */
    uint32_t   n_cov;
    uint32_t   dof;             /* S - n_cov - 2 */
    uint32_t   n_perm;          /* B */
    uint64_t   n_pairs;         /* the sum of n_cis */
    uint8_t   *variant_verdict; /* V: 0 usable, 1 constant, 2 explained by the covariates */
    double    *yy;              /* K */
    double    *gg;              /* V */
    uint32_t  *n_cis;           /* K: the row's pairs */
    double    *perm_r;          /* K x (B + 1), row-major */
    uint32_t  *best_variant;    /* K: an input variant, or RGX_NO_PAIR */
    double    *best_r, *best_slope;   /* K */
    uint32_t  *n_ge;            /* K */
    double    *p_perm;          /* K */
    double    *beta_shape1, *beta_shape2, *p_beta;   /* K */
    uint8_t   *beta_status;     /* K */
    /* statistics */
    uint64_t   n_constant, n_explained, n_flat_rows;
    uint64_t   n_tiles;         /* the device's products of 64 permutations x 64 usable variants: per row ceil((B + 1) / 64) * ceil(n_cis / 64)
                                   (the twin: 0) */
    double     ms_perm;         /* this call, wall */
    double     ms_residual;     /* device time from the first upload to the sample-major residuals (the twin: its residual loops, wall) */
    double     ms_products;     /* device time of the permuted products and the best pairs (the twin: its loops, wall) */
    double     ms_beta;         /* the beta approximation, host wall */
} rgx_qtl_perm_result;
/* out[(B + 1) x S]: row 0 the identity, rows 1 .. B Fisher-Yates shuffles drawn in order from ONE splitmix64 stream: z starts at the seed; next():
 * z += 0x9E3779B97F4A7C15, x = z, x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9, x = (x ^ x >> 27) * 0x94D049BB133111EB, x ^ x >> 31.  A row starts
 * from the identity; for i = S - 1 down to 1: j = (next() * (i + 1)) >> 64 (the 128-bit product), swap p[i] and p[j].  RGX_ERR_ARG for S == 0,
 * S > 65536 or B > 65535. */
int  rgx_qtl_permutations(uint32_t n_samples, uint32_t n_perm, uint64_t seed, uint16_t *out, char *err, size_t errlen);
/* On the cohort's device and stream: the nominal scan's residuals, compaction, G transpose and plan, then one workgroup per (row, 64 permutations)
 * over all the row's tiles of 64 usable variants, a thread per row for the best pair, ONE host wait in front of the copies back, the beta
 * approximation on the host. */
int  rgx_cohort_qtl_permute(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                            const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates,
                            uint32_t window, uint32_t n_perm, const uint16_t *perm, rgx_qtl_perm_result **out, char *err, size_t errlen);
/* Host twin: the same chains in plain C++ (std::fma), the same beta function, no device.  NOT a fallback. */
int  rgx_cohort_qtl_permute_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                                 const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates, uint32_t window,
                                 uint32_t n_perm, const uint16_t *perm, rgx_qtl_perm_result **out, char *err, size_t errlen);
void rgx_cohort_qtl_perm_free(rgx_qtl_perm_result *q);
/* psi(x) and psi'(x) for x > 0 (NaN otherwise), in long double: the recurrence up to x >= 32, then the asymptotic series. */
double rgx_qtl_digamma(double x);
double rgx_qtl_trigamma(double x);
/* The regularised incomplete beta function I_x(a, b), a, b > 0, 0 <= x <= 1 (NaN otherwise): rgx_qtl_pvalue's Lentz fraction with the prefactor
 * exp(a log x + b log1p(-x) - lgammal(a) - lgammal(b) + lgammal(a + b)), in long double; the fraction of (b, a, 1 - x) when x is beyond
 * (a + 1) / (a + b + 2). */
double rgx_qtl_betainc(double x, double a, double b);
/* The beta distribution fitted to p[0 .. n) (each inside (0, 1)) by maximum likelihood, sums in ascending order, long double: mean m and variance
 * v (divisor n); the moment start a = m (m (1 - m) / v - 1), b = a (1 / m - 1); Newton on psi(a) - psi(a + b) = mean log p, psi(b) - psi(a + b) =
 * mean log(1 - p) with the trigamma Jacobian, the step halved while a or b would leave (0, inf), at most 100 steps, done when both relative
 * changes are below 1e-12.  Returns the status of beta_status above (2: n < 2, v == 0 or a moment estimate outside (0, inf); shapes NaN). */
int  rgx_qtl_beta_fit(const double *p, uint32_t n, double *shape1, double *shape2);
/* "phenotype_id\tnum_var\tbeta_shape1\tbeta_shape2\tdof\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\tpval_perm\tpval_beta" and
 * one line per table row that has pairs, in row order: the ID and distance of rgx_cohort_format_qtl for best_variant, num_var = n_cis, doubles as
 * %.17g, NaN as "nan".  q == NULL writes the header line alone; 0 when the arguments do not fit together.  Buffer protocol of
 * rgx_cohort_format_counts. */
size_t rgx_cohort_format_qtl_perm(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph, const rgx_qtl_perm_result *q,
                                  const uint32_t *var_pos, const char *const *variant_id, char *buf, size_t cap);

/* -----------------------------------------------------------------------------------------------------
 * The GROUPED permutation pass: one corrected p per group of table rows -- for a LeafCutter table per intron cluster, whose introns are ratios
 * over one denominator tested against the same variants (FastQTL's --grp, tensorQTL's map_cis(..., group_s=...); neither is available to this
 * project: checked against a restatement in exact rationals and against the ungrouped pass).  The deviations are the ungrouped pass's.
 *   input                 everything rgx_cohort_qtl_permute takes; n_groups = G; group[K]: the row's group in [0, G), or RGX_NO_GROUP for a row
 *                         that takes part in nothing.  A group's members are its rows in ascending table row; they need not be contiguous; a
 *                         group may be empty
 *   errors                RGX_ERR_ARG, before any launch: the ungrouped pass's, with G (B + 1) > 2^32 - 2^16 where it has K (B + 1); G == 0 or
 *                         G > 2^31 - 1; a group[k] >= G that is not RGX_NO_GROUP.  The flag words as in the nominal scan
 *   steps                 basis, dot64, residuals, yy, gg, verdicts, flat rows and cis ranges: the nominal contract's; n_cis[k] as in the ungrouped
 *                         pass (also for a row without a group); group_n_cis[g] = the 64-bit sum of its members' n_cis, n_pairs their sum over
 *                         the groups
 *   per (member k, b, v)  the ungrouped pass's chain and r, with the unpermuted row's own yy[k]
 *   perm_r[g][b]          the largest |r| over all members and their cis variants, compared and stored as bit patterns, b = 0 .. B; +0.0
 *                         throughout for a group without pairs (empty, all members flat, or no member with a cis variant)
 *   best                  of b = 0: best_row[g] (a table row) and best_variant[g] (an input variant) are the pair with the largest bits; on
 *                         equal bits the lowest table row, then the earliest variant; both RGX_NO_PAIR without pairs.  best_r[g] and
 *                         best_slope[g] are that pair's chain: bit for bit the nominal scan's r and slope there; +0.0 without pairs
 *   n_ge .. beta_status   the ungrouped pass's definitions applied to the group's series, dof = S - n_cov - 2
 * No K x (B + 1) array exists anywhere.
 * ----------------------------------------------------------------------------------------------------- */
#define RGX_NO_GROUP 0xffffffffu
/* Owned by the library (rgx_cohort_qtl_group_free), one block, page-locked on the device path. */
typedef struct {
    uint64_t   n_rows;          /* K */
    uint32_t   n_samples;       /* S */
    uint32_t   n_variants;      /* V */
    uint32_t   n_cov;
    uint32_t   dof;             /* S - n_cov - 2 */
    uint32_t   n_perm;          /* B */
    uint32_t   n_groups;        /* G */
    uint64_t   n_pairs;         /* the sum of group_n_cis */
    uint8_t   *variant_verdict; /* V: 0 usable, 1 constant, 2 explained by the covariates */
    double    *yy;              /* K */
    double    *gg;              /* V */
    uint32_t  *n_cis;           /* K: the row's pairs */
    uint32_t  *grp_begin;       /* G + 1: group g's members are grp_row[grp_begin[g] .. grp_begin[g + 1]) */
    uint32_t  *grp_row;         /* grp_begin[G]: table rows, ascending inside a group */
    uint64_t  *group_n_cis;     /* G */
    double    *perm_r;          /* G x (B + 1), row-major */
    uint32_t  *best_row;        /* G: a table row, or RGX_NO_PAIR */
    uint32_t  *best_variant;    /* G: an input variant, or RGX_NO_PAIR */
    double    *best_r, *best_slope;   /* G */
    uint32_t  *n_ge;            /* G */
    double    *p_perm;          /* G */
    double    *beta_shape1, *beta_shape2, *p_beta;   /* G */
    uint8_t   *beta_status;     /* G */
    /* statistics */
    uint64_t   n_constant, n_explained, n_flat_rows;
    uint64_t   n_tiles;         /* the device's products of 64 permutations x 64 usable variants: per member ceil((B + 1) / 64) * ceil(n_cis / 64)
                                   (the twin: 0) */
    double     ms_perm;         /* this call, wall */
    double     ms_residual;     /* device time from the first upload to the sample-major residuals (the twin: its residual loops, wall) */
    double     ms_products;     /* device time of the permuted products and the best pairs (the twin: its loops, wall) */
    double     ms_beta;         /* the beta approximation, host wall */
} rgx_qtl_group_result;
/* group_out[k] = the cluster of ph->row[k] in cl, renumbered 0 .. G - 1 in ascending order of each cluster's first table row; *n_groups = G.
 * RGX_ERR_ARG when a row of ph is no row of cl or is not clustered there. */
int  rgx_cohort_pheno_groups(const rgx_cohort_clusters *cl, const rgx_pheno_table *ph, uint32_t *group_out, uint32_t *n_groups, char *err,
                             size_t errlen);
/* On the cohort's device and stream: the ungrouped pass's stages with one workgroup per (group, 64 permutations) that walks the group's members,
 * a thread per group for the best pair, ONE host wait in front of the copies back, the beta approximation on the host. */
int  rgx_cohort_qtl_permute_grouped(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                    const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov,
                                    const double *covariates, uint32_t window, uint32_t n_perm, const uint16_t *perm, uint32_t n_groups,
                                    const uint32_t *group, rgx_qtl_group_result **out, char *err, size_t errlen);
/* Host twin: the same chains in plain C++ (std::fma), a group a task, the same beta function, no device.  NOT a fallback. */
int  rgx_cohort_qtl_permute_grouped_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                                         const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates, uint32_t window,
                                         uint32_t n_perm, const uint16_t *perm, uint32_t n_groups, const uint32_t *group,
                                         rgx_qtl_group_result **out, char *err, size_t errlen);
void rgx_cohort_qtl_group_free(rgx_qtl_group_result *q);
/* "group_id\tgroup_size\tphenotype_id\tnum_var\tbeta_shape1\tbeta_shape2\tdof\tvariant_id\tdistance\tr\tslope\tslope_se\ttstat\tpval_nominal\t
 * pval_perm\tpval_beta" and one line per group that has pairs, in group order: group_id = clu_<k>_<s> as in the row IDs, of the group's first
 * member; group_size = its member count; phenotype_id and distance those of best_row, num_var = group_n_cis, doubles as %.17g, NaN as "nan".
 * q == NULL writes the header line alone; 0 when the arguments do not fit together.  Buffer protocol of rgx_cohort_format_counts. */
size_t rgx_cohort_format_qtl_group(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph,
                                   const rgx_qtl_group_result *q, const uint32_t *var_pos, const char *const *variant_id, char *buf, size_t cap);

/* -----------------------------------------------------------------------------------------------------
 * The CONDITIONAL permutation pass: the permutation pass of a table row with further variants of its window in the model -- the primitive under
 * tensorQTL's map_independent and QTLtools' conditional pass, neither of which is available to this project: checked against a restatement in
 * exact rationals and against least squares of the full model y ~ 1 + covariates + conditioning variants + g.  In the space the nominal contract
 * has residualised, conditioning on m variants is a rank-m correction of the permutation pass's product:
 *   y'_p . g' = y'_p . g - sum_j (y'_p . z_j)(g . z_j),   z_0 .. z_(m-1) an orthonormal basis of the conditioning residuals.
 * DELIBERATE DEVIATIONS: those of the permutation pass; there is no grouped conditional pass.
 *   input                 everything rgx_cohort_qtl_permute takes; n_series = N conditional SERIES: series c is table row k = series_row[c]
 *                         with the m_c = cond_begin[c + 1] - cond_begin[c] input variants cond_variant[cond_begin[c] ..], in the order given.  A
 *                         row may stand in several series.  The result echoes the lists with cond_begin starting at 0
 *   errors                RGX_ERR_ARG, before any launch: the nominal scan's and the permutations' (with N (B + 1) > 2^32 - 2^16 for the
 *                         result's size); N == 0; a row >= K; m_c == 0 or m_c > RGX_QTL_MAX_COND; S < n_cov + 3 + m_c; a conditioning variant
 *                         >= V, repeated within its series, or not cis to its row; more than 2^32 - 2^16 variants cis to the series' rows in
 *                         all.  RGX_ERR_ARG also for a conditioning variant whose verdict is not 0: the device reports it through a flag word
 *                         beside the nominal scan's two, the twin when it meets it
 *   steps                 basis, dot64, residuals Y[k] with yy, G[v] with gg, verdicts, flat rows and cis ranges: the nominal contract's, unchanged
 *   basis of series c     for j = 0 .. m - 1 in order: v = G[cond_variant_j]; TWICE for i = 0 .. j - 1 in order d = dot64(v, z_i) and v[s] =
 *                         fma(-d, z_i[s], v[s]); nn = dot64(v, v); the series is COLLINEAR (cond_status 1: no pairs, yy_cond +0.0) when
 *                         !(nn > 1e-12 * S) for any j; z_j[s] = v[s] / sqrt(nn), the root and the quotient rounded on their own
 *   row of series c       y' = Y[k]; for j in order d = dot64(y', z_j), y'[s] = fma(-d, z_j[s], y'[s]); yy_cond[c] = dot64(y', y'); the
 *                         series is FLAT (cond_status 2: no pairs) when !(yy_cond > 1e-12 * S)
 *   per usable cis u      of row k (n_window[c] of them, the permutation pass's n_cis[k]): x = G[u]; for j in order beta[c][j][u] = d =
 *                         dot64(x, z_j), x[s] = fma(-d, z_j[s], x[s]); gg'[c][u] = dot64(x, x), from the projected vector and not as gg -
 *                         sum beta^2, which cancels under high LD.  u TAKES PART when gg' > 1e-12 * S: the conditioning variants themselves and
 *                         whatever is in perfect LD with the set drop out here, with no rule of their own.  n_cis[c] = the variants that take part
 *   per (c, b, j)         alpha[c][b][j] = ONE chain acc = fma(y'[perm[b][s]], z_j[s], acc) in ascending s from +0.0
 *   per (c, b, u)         u taking part: dot = ONE chain acc = fma(y'[perm[b][s]], G[u][s], acc) in ascending s from +0.0, then for j = 0 .. m -
 *                         1 in order dot = fma(-alpha[c][b][j], beta[c][j][u], dot); r = dot / sqrt(yy_cond[c] * gg'[c][u]); slope = dot /
 *                         gg'[c][u]
 *   perm_r, best, n_ge, p_perm, beta approximation    the permutation pass's rules per series, with dof[c] = S - n_cov - 2 - m_c: perm_r[c][b] the
 *                         largest |r| as bit patterns, +0.0 throughout without pairs; the best of b = 0 the earliest on ties; beta_status 2
 *                         for a series without pairs
 * ----------------------------------------------------------------------------------------------------- */
#define RGX_QTL_MAX_COND 8
/* Owned by the library (rgx_cohort_qtl_cond_free), one block, page-locked on the device path. */
typedef struct {
    uint64_t   n_rows;          /* K */
    uint32_t   n_samples;       /* S */
    uint32_t   n_variants;      /* V */
    uint32_t   n_cov;
    uint32_t   n_perm;          /* B */
    uint32_t   n_series;        /* N */
    uint32_t   n_cond;          /* cond_begin[N]: the length of cond_variant */
    uint64_t   n_pairs;         /* the sum of n_cis */
    uint8_t   *variant_verdict; /* V: 0 usable, 1 constant, 2 explained by the covariates */
    double    *yy;              /* K */
    double    *gg;              /* V */
    uint32_t  *series_row;      /* N */
    uint32_t  *cond_begin;      /* N + 1, from 0 */
    uint32_t  *cond_variant;    /* n_cond */
    uint8_t   *cond_status;     /* N: 0, 1 collinear, 2 flat */
    double    *yy_cond;         /* N */
    uint32_t  *dof;             /* N: S - n_cov - 2 - m_c */
    uint32_t  *n_window;        /* N: the row's usable cis variants */
    uint32_t  *n_cis;           /* N: those of them that take part; 0 for a collinear or flat series */
    double    *perm_r;          /* N x (B + 1), row-major */
    uint32_t  *best_variant;    /* N: an input variant, or RGX_NO_PAIR */
    double    *best_r, *best_slope;   /* N */
    uint32_t  *n_ge;            /* N */
    double    *p_perm;          /* N */
    double    *beta_shape1, *beta_shape2, *p_beta;   /* N */
    uint8_t   *beta_status;     /* N */
    /* statistics */
    uint64_t   n_constant, n_explained, n_flat_rows;
    uint64_t   n_collinear, n_flat_series;
    uint64_t   n_tiles;         /* the device's products of 64 permutations x 64 usable variants: per series with cond_status 0
                                   ceil((B + 1) / 64) * ceil(n_window / 64) (the twin: 0) */
    double     ms_cond;         /* this call, wall */
    double     ms_residual;     /* device time from the first upload to the sample-major residuals (the twin: its residual loops, wall) */
    double     ms_prepare;      /* device time of the bases, the rows, beta and gg' (the twin: 0, it prepares inside its product loops) */
    double     ms_products;     /* device time of the conditioned products and the best pairs (the twin: its loops, wall) */
    double     ms_beta;         /* the beta approximation, host wall */
} rgx_qtl_cond_result;
/* On the cohort's device and stream: the permutation pass's stages up to the permutations in HBM, then a wave per series for its basis and
 * row, a wave per (series, usable cis variant) for beta and gg', one workgroup per (series, 64 permutations) over all the row's tiles of 64
 * usable variants, a wave per series for n_cis and the best pair, ONE host wait in front of the copies back, the beta approximation on the
 * host. */
int  rgx_cohort_qtl_permute_conditional(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                        const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov,
                                        const double *covariates, uint32_t window, uint32_t n_perm, const uint16_t *perm, uint32_t n_series,
                                        const uint32_t *series_row, const uint32_t *cond_begin, const uint32_t *cond_variant,
                                        rgx_qtl_cond_result **out, char *err, size_t errlen);
/* Host twin: the same chains in plain C++ (std::fma), the same beta function, no device.  NOT a fallback. */
int  rgx_cohort_qtl_permute_conditional_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                                             const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates,
                                             uint32_t window, uint32_t n_perm, const uint16_t *perm, uint32_t n_series, const uint32_t *series_row,
                                             const uint32_t *cond_begin, const uint32_t *cond_variant, rgx_qtl_cond_result **out, char *err,
                                             size_t errlen);
void rgx_cohort_qtl_cond_free(rgx_qtl_cond_result *q);

/* -----------------------------------------------------------------------------------------------------
 * The conditionally independent cis-sQTL signals of every table row: a forward-backward search over the conditional pass -- tensorQTL's
 * map_independent, QTLtools' conditional pass.  One preparation serves the whole call on the device; every round is one conditional pass and
 * one host wait, since the beta fits decide the next round's series.  The decisions are one function for the device path and the twin.
 * DELIBERATE DEVIATIONS: the permutation pass's (no adaptive permutations, no re-estimated dof); no q-values -- the threshold is ONE p for every
 * row, where tensorQTL takes a per-phenotype threshold from the FDR step; no grouped conditional pass.
 *   input                 everything rgx_cohort_qtl_permute takes; p_threshold in (0, 1]; max_signals in 1 .. RGX_QTL_MAX_COND.  RGX_ERR_ARG
 *                         otherwise, and for every error of the two passes
 *   OK(series)            the series (or round-0 row) has pairs (n_cis > 0), beta_status != 2 and p_beta <= p_threshold
 *   round 0               the ungrouped permutation pass as it is.  A row ENTERS when OK; its signal 1 is best_variant
 *   room                  a row with n signals goes another round when n < max_signals and n <= S - n_cov - 3 (the next series' degrees of
 *                         freedom); else it leaves with capped set
 *   forward               each round is ONE conditional pass over the rows still active, in row order, each conditioned on its signals so far
 *                         in order of discovery.  A row whose series is OK appends that series' best variant and stays while it has room;
 *                         otherwise it leaves
 *   backward              ONE conditional pass: for every row with n >= 2 forward signals and every i < n, in (row, i) order, one series
 *                         conditioned on the other n - 1 signals in forward order.  Signal i is KEPT with rank = i + 1 when its series is OK and
 *                         that series' best variant has not been kept for this row by a smaller i; its record is the series'.  A row with
 *                         one forward signal keeps its round-0 record with rank 1 and n_cond 0
 *   result                the kept signals in (row, rank) order, CSR by table row
 * ----------------------------------------------------------------------------------------------------- */
/* Owned by the library (rgx_cohort_qtl_indep_free), one block. */
typedef struct {
    uint64_t   n_rows;          /* K */
    uint32_t   n_samples;       /* S */
    uint32_t   n_variants;      /* V */
    uint32_t   n_cov;
    uint32_t   n_perm;          /* B */
    uint32_t   max_signals;
    double     p_threshold;
    uint64_t   n_signals;       /* sig_begin[K] */
    uint32_t  *sig_begin;       /* K + 1 */
    uint8_t   *capped;          /* K */
    /* per kept signal */
    uint32_t  *variant;         /* an input variant */
    uint32_t  *rank;            /* 1-based place in the row's forward order */
    uint32_t  *n_cond;          /* the variants its record is conditioned on */
    uint32_t  *dof;             /* S - n_cov - 2 - n_cond */
    uint32_t  *n_cis;           /* the variants that took part */
    double    *r, *slope, *p_perm, *beta_shape1, *beta_shape2, *p_beta;
    uint8_t   *beta_status;
    /* statistics */
    uint64_t   n_entered;       /* rows with a signal behind round 0 */
    uint32_t   n_forward_rounds;/* conditional passes going forward */
    uint64_t   n_series_total;  /* conditional series in all, forward and backward */
    uint64_t   n_capped;
    double     ms_indep;        /* this call, wall */
    double     ms_round0, ms_forward, ms_backward;   /* wall, each with its host part */
} rgx_qtl_indep_result;
int  rgx_cohort_qtl_independent(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants,
                                const uint32_t *var_tid, const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates,
                                uint32_t window, uint32_t n_perm, const uint16_t *perm, double p_threshold, uint32_t max_signals,
                                rgx_qtl_indep_result **out, char *err, size_t errlen);
/* Host twin: the same loop over the two host twins, each of which prepares for itself.  NOT a fallback. */
int  rgx_cohort_qtl_independent_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                                     const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates, uint32_t window,
                                     uint32_t n_perm, const uint16_t *perm, double p_threshold, uint32_t max_signals,
                                     rgx_qtl_indep_result **out, char *err, size_t errlen);
void rgx_cohort_qtl_indep_free(rgx_qtl_indep_result *q);
/* rgx_cohort_format_qtl_perm's columns, then "\trank\tn_cond", and one line per kept signal in (row, rank) order: num_var = n_cis, doubles as
 * %.17g, NaN as "nan".  q == NULL writes the header line alone; 0 when the arguments do not fit together.  Buffer protocol of
 * rgx_cohort_format_counts. */
size_t rgx_cohort_format_qtl_indep(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph,
                                   const rgx_qtl_indep_result *q, const uint32_t *var_pos, const char *const *variant_id, char *buf, size_t cap);

/* -----------------------------------------------------------------------------------------------------
 * The trans-sQTL scan of the phenotype table: every table row against every usable variant, genome-wide, keeping only the pairs whose |r| reaches
 * a threshold -- tensorQTL's map_trans, which is not available to this project: checked against a restatement in exact rationals.
 *   input                 everything rgx_cohort_qtl_nominal takes except window, with the same errors; r_min in [0, 1] (NaN or a value outside
 *                         is RGX_ERR_ARG); exclude_cis and exclude_window; max_hits (0: the result's own limit, 2^32 - 2^16)
 *   basis .. variant v    the nominal scan's, unchanged and by the same code: basis, dot64, residuals, yy and the flat rows, gg and the verdicts,
 *                         the usable variants in input order
 *   pairs                 row k meets usable variant v unless the row is flat or -- with exclude_cis -- v is cis to k by the nominal scan's test
 *                         with window = exclude_window (equal tids and start - min(start, exclude_window) <= pos <= end + exclude_window, the
 *                         right side saturating at 2^32 - 1).  n_tested = the pairs that met
 *   per pair              the nominal scan's: ONE chain acc = fma(Y[k][s], G[v][s], acc) in ascending s from +0.0, r = dot / sqrt(yy[k] * gg[v]),
 *                         slope = dot / gg[v] -- for a pair both scans see, the same bits
 *   hit                   a pair that met is a hit when bits(|r|) >= bits(r_min), an integer comparison of the two 64-bit patterns (r is never
 *                         NaN: yy and gg passed their tests).  r_min == +0.0 makes every pair a hit.  No transcendental function runs on the device
 *   result                the hits as a CSR by row: hit_begin[K + 1], hit_variant[H] (an index into the INPUT variants), r[H], slope[H]; a row's
 *                         hits in ascending variant order.  H > max_hits is RGX_ERR_ARG with H in the message, known behind the counting pass
 *                         and before the hit arrays are allocated
 *   threshold             a p-value becomes r_min on the HOST: rgx_qtl_r_threshold below
 *   limits                RGX_ERR_DEVICE when workspace cannot be had.  The device cuts K x V into tiles of 64 rows x 64 usable variants; more
 *                         than 2^31 - 1 tiles is RGX_ERR_ARG
 * ----------------------------------------------------------------------------------------------------- */
/* Owned by the library (rgx_cohort_qtl_trans_free), one block, page-locked on the device path. */
typedef struct {
    uint64_t   n_rows;          /* K */
    uint32_t   n_samples;       /* S */
    uint32_t   n_variants;      /* V */
    uint32_t   n_cov;
    uint32_t   dof;             /* S - n_cov - 2 */
    uint64_t   n_tested;        /* the pairs that met */
    uint64_t   n_hits;          /* H */
    uint8_t   *variant_verdict; /* V: 0 usable, 1 constant, 2 explained by the covariates */
    double    *yy;              /* K */
    double    *gg;              /* V */
    uint32_t  *hit_begin;       /* K + 1 */
    uint32_t  *hit_variant;     /* H */
    double    *r, *slope;       /* H */
    /* statistics */
    uint64_t   n_constant, n_explained, n_flat_rows;
    uint64_t   n_tiles;         /* the device's tiles of 64 rows x 64 variants (the twin: 0) */
    uint64_t   n_hit_tiles;     /* those with a hit, which the device computes twice (the twin: 0) */
    double     ms_trans;        /* this call, wall */
    double     ms_residual;     /* device time from the first upload to the sample-major residuals (the twin: its residual loops, wall) */
    double     ms_count;        /* device time of the counting pass over every tile up to its totals (the twin: its pair loops, wall) */
    double     ms_emit;         /* device time from the hit tiles' products to the hits in order (the twin: 0) */
} rgx_qtl_trans_result;
/* On the cohort's device and stream: the nominal scan's stages up to the sample-major residuals, one workgroup per (64 rows, 64 usable variants)
 * that counts its hits, 64-bit totals and two scans, ONE host wait for H, then one workgroup per tile with hits, a stable sort on the row and
 * the copies back. */
int  rgx_cohort_qtl_trans(rgx_cohort *co, const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                          const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates, double r_min, int exclude_cis,
                          uint32_t exclude_window, uint64_t max_hits, rgx_qtl_trans_result **out, char *err, size_t errlen);
/* Host twin: the same chains in plain C++ (std::fma), rows shared among threads, no device.  NOT a fallback. */
int  rgx_cohort_qtl_trans_host(const rgx_pheno_table *ph, const rgx_qtl_region *regions, uint32_t n_variants, const uint32_t *var_tid,
                               const uint32_t *var_pos, const int8_t *dosage, uint32_t n_cov, const double *covariates, double r_min,
                               int exclude_cis, uint32_t exclude_window, uint64_t max_hits, rgx_qtl_trans_result **out, char *err, size_t errlen);
void rgx_cohort_qtl_trans_free(rgx_qtl_trans_result *q);
/* The smallest double r in [0, 1] with rgx_qtl_pvalue(rgx_qtl_tstat(r, dof), dof) <= p, by bisection on the 64-bit patterns between +0.0 and 1.0:
 * the low end fails, the high end passes, the high end is returned -- the definition is this algorithm.  p >= 1 gives +0.0; p < 0, a NaN p and
 * dof == 0 give NaN. */
double rgx_qtl_r_threshold(double p, uint32_t dof);
/* "phenotype_id\tvariant_id\tr\tslope\tslope_se\ttstat\tpval" and one line per hit in CSR order; IDs and number formats of rgx_cohort_format_qtl.
 * q == NULL writes the header line alone; 0 when the arguments do not fit together.  Buffer protocol of rgx_cohort_format_counts. */
size_t rgx_cohort_format_qtl_trans(const rgx_cohort_matrix *m, const rgx_cohort_clusters *cl, const rgx_pheno_table *ph,
                                   const rgx_qtl_trans_result *q, const uint32_t *var_pos, const char *const *variant_id, char *buf, size_t cap);

/* The genotypes of a cohort's samples from a VCF (plain, gzip, bgzip) or a BCF, as rgx_cohort_qtl_nominal takes them.  Samples are matched to
 * m->sample_name BY NAME; a cohort sample the file does not have is RGX_ERR_ARG, "Sample <name> has no genotypes in <file>".  A record is
 * skipped, and counted, when it is multi-allelic (anything but one ALT), carries no GT, or lies on a contig m does not know.  The dosage is the
 * number of non-reference alleles of a diploid GT call; a missing allele, or a ploidy other than 2, gives -1.  The variants are sorted stably
 * by (cohort contig, position); id is the ID column, or <contig>:<pos>:<ref>:<alt> when that is ".". */
typedef struct {
    uint32_t   n_variants, n_samples;
    uint32_t  *tid, *pos;       /* n_variants: the cohort's contig, the 1-based position */
    int8_t    *dosage;          /* n_variants * n_samples, variant-major, the cohort's sample order */
    char     **id;              /* n_variants */
    uint64_t   n_records, n_multiallelic, n_no_gt, n_unknown_contig;
} rgx_genotypes;
int  rgx_genotypes_load(const char *path, const rgx_cohort_matrix *m, rgx_genotypes **out, char *err, size_t errlen);
void rgx_genotypes_free(rgx_genotypes *g);

/* Library/build identification: "regtools_amd <version> gfx950". */
const char *rgx_version(void);

/* Stage-level kernel entry points on caller-provided DEVICE buffers (used by tests/bench to measure the
 * dominant kernel in isolation; all asynchronous on `stream`, a hipStream_t passed as void*). */
typedef struct { uint64_t cpos, upos; uint32_t clen, isize; } rgx_member;   /* == rgx::Member */
int  rgx_k_inflate(const void *d_comp, const rgx_member *d_members, uint32_t n_members,
                   void *d_arena, uint32_t *d_status, void *stream);
/* The same with the form of the decoder named: 0 = the pipeline's choice (one member per WAVE, whole member in LDS, up to 2048 members -- a
 * member in ~1.5 ms; above that one member per LANE -- ~8 ms per launch whatever its size, 196,608 members at a time; REGTOOLS_AMD_INFLATE=
 * lane|wave|ring|coop overrides), 1 = lane (k_inflate), 2 = wave (k_inflate_wave), 3 = lane with an LDS window and whole-line output
 * (k_inflate_ring; needs 16 readable bytes in front of d_arena), 4 = lane with the long matches copied by the wave (k_inflate_coop: what the
 * pipeline runs above 2048 members; the members of a launch must lie in the arena in the order of the list, a group of 1024 of them within
 * 4 GiB -- a list that does not is refused by forms 0 and 4: d_status[0] = the first offending member, d_status[1] = 10, nothing written),
 * 5 = lane taking up to four literals per trip (k_inflate<.., 4>). */
int  rgx_k_inflate_form(int form, const void *d_comp, const rgx_member *d_members, uint32_t n_members,
                        void *d_arena, uint32_t *d_status, void *stream);

/* The tail behind the DEFLATE launch, stage by stage (tests): the exclusive scan, the radix sort and the group-by every table goes through, on the
 * caller's DEVICE arrays.  They run the pipeline's own code on the context's stream with scratch carved from the context's buffers as the
 * pipeline carves it, and return behind a synchronisation of that stream; the caller's arrays must be complete before the call (the
 * context's stream does not wait for the caller's).  RGX_ERR_DEVICE also when a stage wrote behind the scratch its own sizing function
 * (scan_tmp_words / radix_tmp_words) gives it. */
/* d_out[i] = d_in[0] + ... + d_in[i - 1] (mod 2^32); d_out may be d_in; *d_total = the sum of all n, written only when d_total is not NULL
 * (0 for n = 0). */
int  rgx_k_scan_u32(rgx_ctx *ctx, const uint32_t *d_in, uint32_t *d_out, uint32_t n, uint32_t *d_total, char *err, size_t errlen);
/* The front of the pipeline on its own (tests): BGZF member discovery on a file that lies in HBM, as rgx_extract_device runs it -- d_bam readable to
 * bam_len + 8.  Every offset o with o + 18 <= bam_len that carries the ten fixed bytes of a BGZF header is a candidate; the members are the
 * candidates that chain up (BSIZE + 1) from offset 0, and with root2 != ~0 -- a second pass over the same candidates and buffers, as behind a seek
 * the first chain does not reach -- also those that chain up from root2; cpos = o + 18, clen clipped to cpos + clen + 8 <= bam_len, isize the
 * footer's (~0: the header runs past the file or BSIZE + 1 < 26; such a candidate is listed and ends its chain), upos the running sum of the
 * sizes <= 65536.  d_true_sizes (device, one per member, or NULL) replaces the footers' sizes before the sum.  q_index[k] / q_upos[k]: the
 * member whose header starts at q_coff[k] (n_members and ~0 when there is none); stop: the first member at or behind q_index[0] that is empty
 * or larger than 65536 (0xffffffff: none).  bam_len == 0 or a file without candidates gives counts of 0, not an error.  RGX_ERR_DEVICE also
 * when the candidate fill or the member fill wrote behind its count. */
typedef struct {
    uint64_t n_candidates, n_members, total_inflated;
    uint64_t *candidates; rgx_member *members;
    uint64_t q_upos[3]; uint32_t q_index[3], stop;
} rgx_members_result;
int  rgx_k_members(rgx_ctx *ctx, const void *d_bam, uint64_t bam_len, uint64_t root2, const uint32_t *d_true_sizes, const uint64_t *q_coff,
                   rgx_members_result **out, char *err, size_t errlen);
void rgx_members_result_free(rgx_members_result *r);
/* d_perm_out = the positions 0 .. n-1 in stable order of the key whose word k (k = 0 the LEAST significant) is the low nbits[k] (1 .. 32) bits of
 * d_words[k][position]; d_words and nbits are host arrays of n_words entries.  mode = how the sort is driven, word by word: 0 = plain passes that
 * gather the word through the permutation, 1 = the word gathered once and its passes keyed, 2 = keyed passes on a word the caller's gather
 * produces (here: the column through the permutation, or a copy of it in front of the first pass).  n_scratch (0 = n): the key count the scratch
 * is sized and carved for, n_scratch >= n -- a merge sorts its unique rows in the scratch of all its rows.  n = 0 writes nothing. */
int  rgx_k_radix_sort(rgx_ctx *ctx, uint32_t n, uint32_t n_scratch, uint32_t n_words, const uint32_t *const *d_words, const uint32_t *nbits,
                      int mode, uint32_t *d_perm_out, char *err, size_t errlen);
/* Junction events (file order) -> the unique rows in output order.  Key = (tid, start, ilen_cls), ilen_cls = intron length << 2 | strand class;
 * every tid is below n_groups and 2^group_bits, every ilen_cls below 2^ilen_bits; rank_of_group_host[tid] (host, n_groups entries) leads the
 * output order.  form: 0 = equal keys grouped per tile of events first (junctions extract), 1 = the events sorted as they are (identify),
 * 2 = 1 + the row map of -b: d_ev_urow[event] = its unique row, d_urow_pos[unique row] = that row's place in the output (n_events entries
 * each).  d_rows_out: room for 10 x n_events words; receives ten columns of *n_rows_out entries each -- tid, start, end, thick_start,
 * thick_end, count, name rank (1-based, by first event), first event, last event, strand byte of the last event.  The context's last
 * table is no longer valid for rgx_last_table_pack_device afterwards. */
int  rgx_k_group_by(rgx_ctx *ctx, const uint32_t *d_tid, const uint32_t *d_start, const uint32_t *d_ilen_cls, const uint32_t *d_ts,
                    const uint32_t *d_te, const uint8_t *d_strand, uint32_t n_events, uint32_t group_bits, uint32_t ilen_bits,
                    const uint32_t *rank_of_group_host, uint32_t n_groups, int form, uint32_t *d_rows_out, uint64_t *n_rows_out,
                    uint32_t *d_ev_urow, uint32_t *d_urow_pos, char *err, size_t errlen);
/* The component search of the cohort's intron clusters on the caller's edge list: edge e joins vertices d_a[e] and d_b[e], all below
 * n_vertices (self loops and duplicates allowed).  d_label_out[v] = the smallest vertex id of v's component; *n_rounds = the hook + jump
 * rounds run, the one that changed nothing included. */
int  rgx_k_components(rgx_ctx *ctx, uint32_t n_vertices, uint32_t n_edges, const uint32_t *d_a, const uint32_t *d_b, uint32_t *d_label_out,
                      uint32_t *n_rounds, char *err, size_t errlen);

/* The interval kernels of `cis-splice-effects identify / associate` and the two annotate commands, stage by stage (tests): the junction scan
 * (a11), the window join's pair lists (a9) and `associate`'s pair join on the caller's own junctions, events and windows.  (The variant scan,
 * a10, has had its entry all along: rgx_variant_windows, below.)  Each runs the half its command runs, on the context's stream, with the
 * variable-length outputs in scratch that has guard words behind every list: RGX_ERR_DEVICE when a fill pass wrote more than its count pass
 * counted.  Results are malloc'ed host arrays, freed by the matching *_free. */
typedef struct rgx_gtf rgx_gtf;
/* 1: the annotation carries the direct (contig, bin) index, 0: the kernels find a bin's transcripts by binary search (the model builds the
 * index only while contigs x (largest bin + 1) <= 2^23). */
int  rgx_gtf_bin_index(const rgx_gtf *g);
/* a11 as the kernel leaves it: junction i (contig = index into the annotation's contigs or -1, start, end1 = Junction.end + 1, strand byte)
 * -> flags (bit0 known_donor, bit1 known_acceptor, bit2 known_junction), visits (exon records of its candidate transcripts; form 1 counts all
 * junctions into visits_total only and leaves visits 0) and its items item_off[i] .. item_off[i + 1]: (kind, a, b) in the order written, kind
 * 0 = transcript a listed, 1 = exon a-b skipped, 2 = donor a skipped, 3 = acceptor a skipped; duplicates are NOT removed
 * (rgx_annotate_junctions does that).  keep_single: `junctions annotate -S`.  form: 0 = one wave per junction, 1 = one lane per junction. */
typedef struct {
    uint64_t n, visits_total; uint32_t *flags, *visits, *item_off, *item_kind, *item_a, *item_b;
} rgx_junction_items;
int  rgx_k_junction_scan(rgx_ctx *ctx, const rgx_gtf *g, uint64_t n, const int32_t *contig, const uint32_t *start, const uint32_t *end1,
                         const char *strand, int keep_single, int form, rgx_junction_items **out, char *err, size_t errlen);
void rgx_junction_items_free(rgx_junction_items *r);
/* n pairs (first[k], window[k]), window-major; n_batches = the batches they were made in (1 for rgx_k_assoc_pairs) */
typedef struct { uint64_t n; uint32_t n_batches; uint32_t *first, *window; } rgx_pair_list;
void rgx_pair_list_free(rgx_pair_list *r);
/* a9: events as DEVICE columns (tid, read pos, read end; sorted by (tid, pos); complete before the call), windows (tid, beg, end) as host
 * arrays -> pairs (event, window): for window w in order the events with tid == w_tid, rpos < end, rend > beg (signed 32-bit compares) in
 * event order.  pair_batch: the lists are made in batches of whole windows of at most this many pairs (a larger window is a batch of its own);
 * 0 = the product's size (2^26, or REGTOOLS_AMD_PAIR_BATCH). */
int  rgx_k_window_pairs(rgx_ctx *ctx, const uint32_t *d_tid, const uint32_t *d_rpos, const uint32_t *d_rend, uint32_t n_events, uint32_t n_windows,
                        const int32_t *w_tid, const int32_t *w_beg, const int32_t *w_end, uint64_t pair_batch, rgx_pair_list **out, char *err,
                        size_t errlen);
/* `associate`: windows (contig index or -1, cis range [ces, cee]) against junctions bucketed by contig (contig_off: n_contigs + 1 host entries;
 * start / end in bucket order) -> pairs (junction, window): window w keeps the junctions of its contig whose start or end lies in [ces, cee]. */
int  rgx_k_assoc_pairs(rgx_ctx *ctx, uint32_t n_windows, const int32_t *w_contig, const uint32_t *w_ces, const uint32_t *w_cee, uint32_t n_contigs,
                       const uint32_t *contig_off, uint32_t n_junctions, const uint32_t *j_start, const uint32_t *j_end, rgx_pair_list **out,
                       char *err, size_t errlen);

/* =====================================================================================================
 * `cis-splice-effects identify`.
 * Replaces CisSpliceEffectsIdentifier::identify() + annotate_junctions()
 * (src/cis-splice-effects/cis_splice_effects_identifier.cc:222-312) and the interval cores it drives:
 * VariantsAnnotator::annotate_record_with_transcripts (src/variants/variants_annotator.cc:455-518),
 * the per-variant JunctionsExtractor re-runs (identifier.cc:288-299) and
 * JunctionsAnnotator::annotate_junction_with_gtf (src/junctions/junctions_annotator.cc:344-363).
 * ===================================================================================================== */
typedef struct {
    const char *vcf_path, *bam_path, *fasta_path, *gtf_path;   /* the four positional arguments (identifier.cc:193-198) */
    const char *out_tsv;       /* -o  annotated junctions; NULL = stdout */
    const char *out_vcf;       /* -v  splice-relevant variants (VCF); NULL = not written */
    const char *out_bed;       /* -j  junctions BED12; NULL = not written */
    uint32_t    window;        /* -w  [0 = the cis-effect window between neighbouring exons] */
    uint32_t    intronic_min;  /* -i  [2] */
    uint32_t    exonic_min;    /* -e  [3] */
    int32_t     all_intronic;  /* -I */
    int32_t     all_exonic;    /* -E */
    int32_t     skip_single;   /* 1 unless -S */
    int32_t     strandness;    /* -s  0 XS, 1 RF, 2 FR, 3 intron-motif */
    char        strand_tag[2]; /* -t */
    uint32_t    min_anchor;    /* -a  (also the minimum intron length here: ctor quirk junctions_extractor.h:200) */
    uint32_t    min_intron;    /* -m  accepted and ignored, as upstream */
    uint32_t    max_intron;    /* -M */
    int32_t     override_motif;/* -C */
    const char *bed_path;      /* rgx_associate only: junctions BED12 (second positional of `cis-splice-effects associate`) */
    int32_t     echo;          /* 1: write to stderr what upstream writes while it works -- "exonic_min_distance_ is 3" (variants_annotator.h:151), and per
                                * splice-relevant variant "Variant <chrom> <start> <end> <score>" + "Variant region is <region>" (identifier.cc:265-277,
                                * associator.cc:243-257); the tool sets it, a library caller normally does not [0] */
} rgx_identify_params;

typedef struct {
    uint64_t n_variants, n_relevant, n_windows, n_pairs, n_window_rows, n_junctions;
    uint64_t n_records, n_events;
    uint64_t exon_visits_variants;   /* E_v summed: exon records of all candidate transcripts (SURVEY 8d algorithmic bytes) */
    uint64_t exon_visits_junctions;  /* E_j summed */
    double   ms_total, ms_gtf, ms_variants, ms_extract, ms_join, ms_annotate, ms_output;
    double   ms_k_variant_scan, ms_k_junction_scan, ms_k_window_pairs;   /* the interval kernels alone (HIP events, both passes of each) */
} rgx_identify_stats;

void rgx_identify_params_default(rgx_identify_params *p);   /* CisSpliceEffectsIdentifier ctor, identifier.h:101-117 */

/* Whole command: reads the four files, runs the interval kernels and the extraction on the device, writes -o/-v/-j.
 * Error texts and the exit-code mapping are the reference's (nonzero return == exit 1). */
int  rgx_identify(rgx_ctx *ctx, const rgx_identify_params *p, rgx_identify_stats *stats, char *err, size_t errlen);
/* The same over several devices: the BAM's extraction is sharded over `devices` the way rgx_extract_multi shards it (contiguous member
 * ranges cut at record starts from the index), the junction events are gathered onto devices[0] in file order with device-to-device copies, and the
 * join, the annotation and the outputs run there.  Contexts come from the process-wide cache rgx_extract_multi uses; a device may be listed more than
 * once.  Outputs are byte-identical to rgx_identify's whatever the list. */
int  rgx_identify_multi(const int *devices, int n_devices, const rgx_identify_params *p, rgx_identify_stats *stats, char *err, size_t errlen);

/* SURVEY 8(f) rows f2/f3 -- the three sibling commands over the same kernels.
 * `cis-splice-effects associate` (CisSpliceEffectsAssociator::associate, cis_splice_effects_associator.cc:234-276): the junctions come
 * from p->bed_path (BED12, e.g. the output of `junctions extract`) instead of a BAM; bam_path/strandness/strand_tag are ignored. */
int  rgx_associate(rgx_ctx *ctx, const rgx_identify_params *p, rgx_identify_stats *stats, char *err, size_t errlen);
/* `variants annotate` (VariantsAnnotator::annotate_vcf, variants_annotator.cc:541-550): EVERY record of p->vcf_path written to
 * p->out_vcf (NULL = stdout) with genes= transcripts= distances= annotations= appended to INFO ("NA" when not splice relevant).
 * Uses vcf_path, gtf_path, out_vcf, intronic_min, exonic_min, all_intronic, all_exonic, skip_single. */
int  rgx_variants_annotate(rgx_ctx *ctx, const rgx_identify_params *p, rgx_identify_stats *stats, char *err, size_t errlen);
/* `junctions annotate` (junctions_main.cc:62-93): BED12 rows -> annotated TSV (out_path NULL = stdout); *n_rows = rows written.
 * bedtools' reader semantics are kept: leading #/track/browser lines are skipped, a later one (or a blank line) ends the input,
 * a malformed line ends the run with the reference's message after the rows before it were written. */
int  rgx_junctions_annotate(rgx_ctx *ctx, const char *bed_path, const char *fasta_path, const char *gtf_path, const char *out_path,
                            uint64_t *n_rows, char *err, size_t errlen);
/* The same with options.  Bit 0 = -S (junctions_annotator.cc:392-393, consumed at :131 / :231): single-exon transcripts take part in the scan (they
 * can make a junction's donor or acceptor known, never skip anything); the reference's one unchecked read on this path (exons[i + 1] behind a
 * transcript's last exon, with or without -S) is "no match" here, as in the default mode.  Bit 1 = echo: "position = <region>" on stderr for each of
 * a junction's two FASTA look-ups, as get_reference_sequence writes it (junctions_annotator.cc:366-370); the tool sets it. */
#define RGX_ANNOTATE_SINGLE_EXON 1
#define RGX_ANNOTATE_ECHO        2
int  rgx_junctions_annotate_opts(rgx_ctx *ctx, const char *bed_path, const char *fasta_path, const char *gtf_path, const char *out_path,
                                 int options, uint64_t *n_rows, char *err, size_t errlen);

/* Stage entry points over a loaded annotation (flat exon/transcript/bin arrays in HBM; rgx_gtf is declared with the rgx_k_* entries above). */
int  rgx_gtf_load(rgx_ctx *ctx, const char *gtf_path, rgx_gtf **out, char *err, size_t errlen);   /* GtfParser::load, gtf_parser.cc:257-263 */
void rgx_gtf_free(rgx_gtf *g);
int  rgx_gtf_info(const rgx_gtf *g, uint32_t *n_transcripts, uint32_t *n_exons, uint32_t *n_chroms);
int  rgx_gtf_transcript_bin(const rgx_gtf *g, const char *transcript_id, uint32_t *bin);           /* GtfParser::bin_from_transcript */

/* a10: one row per variant (chrom name + 0-based pos).  hit_off has n+1 entries; hits are in the reference's
 * visitation order; annotation codes 1 exonic, 2 intronic, 3 splicing_exonic, 4 splicing_intronic. */
typedef struct {
    uint64_t n; uint32_t *cis_start, *cis_end; uint32_t *hit_off; uint32_t *hit_transcript, *hit_annotation, *hit_distance;
} rgx_variant_hits;
int  rgx_variant_windows(rgx_ctx *ctx, const rgx_gtf *g, uint64_t n, const char *const *chrom, const uint32_t *pos0, uint32_t intronic_min,
                         uint32_t exonic_min, int all_intronic, int all_exonic, int skip_single, rgx_variant_hits **out, char *err, size_t errlen);
void rgx_variant_hits_free(rgx_variant_hits *h);
const char *rgx_gtf_transcript_id(const rgx_gtf *g, uint32_t t);

/* a11: one row per junction (chrom, start, end = Junction.end + 1, strand).  flags bit0 known_donor, bit1 known_acceptor,
 * bit2 known_junction; counts are of UNIQUE skipped elements; transcripts in id order, offsets n+1. */
typedef struct {
    uint64_t n; uint32_t *flags, *n_acceptors_skipped, *n_exons_skipped, *n_donors_skipped; uint32_t *tx_off, *tx;
} rgx_junction_annot;
int  rgx_annotate_junctions(rgx_ctx *ctx, const rgx_gtf *g, uint64_t n, const char *const *chrom, const uint32_t *start, const uint32_t *end1,
                            const char *strand, rgx_junction_annot **out, char *err, size_t errlen);
void rgx_junction_annot_free(rgx_junction_annot *a);

/* a9: the window join on its own.  For every window w (contig name, 0-based half-open [beg, end) as sam_itr_querys leaves a region)
 * the junction table that `junctions extract -r` over that window would produce with the parameters in p (p->region is ignored):
 * only reads with pos < end && endpos > beg count, so read_count / thick bounds / names are window-restricted.  The BAM is inflated
 * and scanned ONCE for all windows.  Rows come window-major in input order, inside a window in get_all_junctions order; name_index
 * restarts at 1 in every window.  A contig that is not in the BAM header is an error (RGX_ERR_REGION), as upstream. */
typedef struct {
    uint64_t n;
    uint32_t *window, *start, *end, *thick_start, *thick_end, *read_count, *name_index;
    char *strand;
} rgx_window_rows;
int  rgx_window_join(rgx_ctx *ctx, const char *bam_path, const rgx_extract_params *p, uint64_t n_windows, const char *const *chrom,
                     const int32_t *beg, const int32_t *end, rgx_window_rows **out, char *err, size_t errlen);
void rgx_window_rows_free(rgx_window_rows *r);

#ifdef __cplusplus
}
#endif
#endif
