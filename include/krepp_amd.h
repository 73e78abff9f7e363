/*
 * krepp_amd.h — C-ABI of the MI355X-native `krepp dist` query path.
 *
 * The reference (bo1929/krepp v0.8.3) has no FFI/plugin layer; its drop-in
 * surfaces are the CLI, the on-disk index, and one internal seam:
 *
 *     IBatch(index, qs, hdist_th, chisq, dist_max, tau, no_filter, multi, summarize)
 *     IBatch::estimate_distances(std::stringstream&)          src/query.hpp:49-63
 *
 * constructed per 512-read batch on the reader thread and run inside an OpenMP
 * task (src/krepp.cpp:365-383).  This header is that seam as a C ABI: plain
 * pointers and sizes, no C++ or torch types.  Each entry point names the
 * reference interface it replaces.  Every function returns 0 on success or a
 * negative kr_status; kr_last_error() returns a per-thread message.
 *
 * Ownership: the caller owns every host buffer it passes in; the library owns
 * all device memory and every buffer it returns (valid until the owning handle
 * is destroyed or, for results, until the next submit on the same stream).
 * A kr_index is immutable after upload and may be shared by any number of
 * kr_stream objects; a kr_stream is used by one host thread at a time.
 *
 * There is NO CPU fallback: without a usable HIP device every device entry
 * point returns KR_ERR_NO_DEVICE.
 */
#ifndef KREPP_AMD_H
#define KREPP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KR_API __attribute__((visibility("default")))

typedef enum kr_status {
  KR_OK = 0,
  KR_ERR_ARG = -1,        /* bad argument / unsupported configuration          */
  KR_ERR_IO = -2,         /* index directory / file problems ([ERROR] paths of  */
                          /* src/index.cpp:51-158, src/krepp.cpp:66-108)        */
  KR_ERR_FORMAT = -3,     /* inconsistent index files, incompatible libraries  */
  KR_ERR_NO_DEVICE = -4,  /* no HIP device / HIP runtime failure               */
  KR_ERR_NOMEM = -5,
  KR_ERR_CAPACITY = -6,   /* a device-side buffer overflowed; resubmit smaller  */
  KR_ERR_STATE = -7,      /* call order (collect without submit, ...)           */
  KR_ERR_UNSUPPORTED = -8 /* this batch cannot be served this way; use the general call (kr_batch_collect_text) */
} kr_status;

#define KR_MAX_HDIST_TH 16u /* k-h <= 16 (src/krepp.hpp:77-79): hd never exceeds 16 */

/* ------------------------------------------------------------------------- */
/* Host-side index: replaces TargetIndex::load_index (src/krepp.cpp:66-108),   */
/* Index::load_partial_index / load_partial_tree / generate_partial_tree /     */
/* make_rho_partial (src/index.cpp:3-158,188-201), FlatHT::load                */
/* (src/table.cpp:65-75), CRecord::load (src/record.cpp:203-211), Tree::load   */
/* and Node::parse / generate_tree (src/phytree.cpp:150-253,394-404).          */
/* ------------------------------------------------------------------------- */
typedef struct kr_host_index kr_host_index;

/* One partial library as laid out on disk (little-endian, no padding). */
typedef struct kr_lib_view {
  const uint64_t* inc;   /* inc-*    payload: cumulative bucket END offsets [nrows]  */
  const uint32_t* cmer;  /* cmer-*   payload: interleaved (enc32, se) [2*nkmers]     */
  const uint32_t* pse;   /* crecord-* se_to_pse: interleaved (first, second) [2*nsubsets] */
  const double* rho;     /* crecord-* se_to_rho [nnodes], already scaled by            */
                         /* make_rho_partial's (#residues present)/m                    */
  uint64_t nkmers;
  uint32_t nrows;
  uint32_t nsubsets;
  uint32_t nnodes;       /* crecord's nnodes = tree nodes + 1                           */
  uint32_t r;            /* metadata-* r                                                */
  uint32_t frac;         /* metadata-* frac                                             */
  uint32_t w;            /* metadata-* w (informational)                                */
} kr_lib_view;

typedef struct kr_index_view {
  uint32_t k, h, m;
  const uint8_t* ppos;       /* [h]   LSH positions, descending (metadata-*)           */
  const uint8_t* npos;       /* [k-h] non-LSH positions, ascending                     */
  uint32_t nlibs;
  const kr_lib_view* libs;
  uint32_t tree_nnodes;      /* Tree::nnodes; colour ids 1..tree_nnodes are tree nodes */
  const uint8_t* node_kind;  /* [tree_nnodes+1] 0 = null (Tree::get_node == nullptr),  */
                             /* 1 = leaf, 2 = internal (src/query.cpp:371-381)         */
  uint32_t wbackbone;        /* Index::check_wbackbone                                 */
} kr_index_view;

KR_API int kr_host_index_load(const char* index_dir, kr_host_index** out);
/* `krepp seek` (src/sketch.cpp:3-39): a single-reference sketch file presented as an index with one library
 * and a one-leaf tree, so that kr_index_upload / kr_stream_* / kr_batch_* serve it unchanged. */
KR_API int kr_host_sketch_load(const char* sketch_path, kr_host_index** out);
KR_API void kr_host_index_free(kr_host_index*);
KR_API int kr_host_index_view(const kr_host_index*, kr_index_view* out);
/* Node::get_name (src/phytree.hpp:134-145): label, or se-1 for unlabelled nodes. */
KR_API const char* kr_host_index_node_name(const kr_host_index*, uint32_t se);
/* the label as written in the Newick / reflist ("" for unlabelled nodes) */
KR_API const char* kr_host_index_node_label(const kr_host_index*, uint32_t se);
KR_API uint32_t kr_host_index_node_parent(const kr_host_index*, uint32_t se);
KR_API double kr_host_index_node_blen(const kr_host_index*, uint32_t se);

/* ------------------------------------------------------------------------- */
/* Device index: the read-only state IBatch borrows from Index                 */
/* (Index::check_partial src/index.hpp:27, Index::bucket_indices               */
/* src/index.cpp:160-168, Index::get_crecord :170, LSHF::compute_hash /        */
/* drop_ppos_lr src/lshf.cpp:62-69).                                           */
/* ------------------------------------------------------------------------- */
typedef struct kr_index kr_index;

#define KR_VIEW_HOST 0u
#define KR_VIEW_DEVICE 1u /* the view's inc/cmer/pse/rho pointers are device pointers */

/* Re-lays the on-disk arrays out for the GPU (DESIGN.md "HBM layout") in HBM of
 * `device`.  With KR_VIEW_DEVICE the big arrays are read from device memory
 * (ppos/npos/node_kind and the kr_lib_view structs themselves stay host). */
KR_API int kr_index_upload(const kr_index_view* view, int device, uint32_t flags, kr_index** out);
KR_API void kr_index_free(kr_index*);

/* Flat device buffers of an uploaded index, for replication to other GPUs by
 * whatever transport the host uses (RCCL broadcast from torch.distributed,
 * hipMemcpyPeer, ...).  `desc` is a small host blob describing sizes and
 * parameters; kr_index_import allocates the same buffers on another device and
 * returns their addresses so the transport can fill them. */
typedef struct kr_index_buffer {
  void* dptr;
  uint64_t bytes;
} kr_index_buffer;
KR_API int kr_index_export(const kr_index*, void* desc, uint64_t* desc_bytes, kr_index_buffer* bufs, uint32_t* nbufs);
KR_API int kr_index_import(const void* desc, uint64_t desc_bytes, int device, kr_index** out, kr_index_buffer* bufs,
                           uint32_t* nbufs);
KR_API uint64_t kr_index_device_bytes(const kr_index*);
/* Words (4 bytes) per slot of the slotted copy of the bucket heads the upload made for this index, 0 when it kept the packed
 * table only (sparse tables; INTEGRATION.md "Memory and tuning knobs").  Says which scan kernel serves the index:
 * kr_scan_pipe_kernel_t (slotted) or kr_scan_kernel_t (packed). */
KR_API uint32_t kr_index_slot_words(const kr_index*);
/* The slot format itself: 0 packed table only; 5 / 6 / 7 / 8 slots of 32 / 64 / 128 / 48 four-byte words (kr_scan_pipe_kernel_t);
 * 9 FILTER slots -- two 128-byte lines of 24-bit codes per row, one line per probe for most buckets, candidates verified by
 * the accumulate kernel (kr_scan_filt_kernel_t; replaces the linear bucket scan of src/query.cpp:361-368). */
KR_API uint32_t kr_index_slot_format(const kr_index*);
/* The packed scan's shape and front: log2 of the lanes that share a probe (0, 2 or 3: from the mean bucket length, or KR_LOG_G at
 * upload), and whether the packed tables carry the row-occupancy bitmap (sparse tables, or KR_OCC_BITMAP at upload). */
KR_API uint32_t kr_index_log_g(const kr_index*);
KR_API uint32_t kr_index_occ_bitmap(const kr_index*);

/* Replicate an uploaded index into the HBM of `ndev` more devices of this node by RCCL broadcast
 * (ncclBroadcast per flat buffer, one communicator over the root's device and the targets, xGMI):
 * the index crosses PCIe once, whatever the number of GPUs.  Load time only; there is no collective
 * on the query path.  Replaces what the reference does once per process, TargetIndex::load_index
 * (src/krepp.cpp:92-106), for the GPUs after the first.  replicas[i] lives on devices[i] and is freed
 * with kr_index_free; devices are distinct; a device equal to the root's gives a second copy in the
 * same HBM (one-rank communicator).  RCCL (librccl.so.1) is loaded on first use.  RCCL may print a version
 * banner on stdout when the first communicator is made: the library never touches the process's file
 * descriptors, so an application whose stdout carries the report redirects it around this call itself,
 * before its writer threads start. */
KR_API int kr_index_broadcast(const kr_index* root, int ndev, const int* devices, kr_index** replicas);

/* ------------------------------------------------------------------------- */
/* Query: IBatch ctor + IBatch::estimate_distances (src/query.cpp:8-38,        */
/* 141-156): search_mers (:40-94), IMers::add_matching_mer (:352-390),         */
/* Minfo::update_match (src/query.hpp:153-176), summarize_matches              */
/* (src/query.cpp:96-139), Minfo::optimize_likelihood (:426-433) with          */
/* HDistHistLLH (src/hdhistllh.hpp:51-96) and Boost's brent_find_minima, and   */
/* the selection logic of report_distances (:158-196).                         */
/* ------------------------------------------------------------------------- */
typedef struct kr_params {
  uint32_t hdist_th;   /* --hdist-th  [4]      (src/krepp.hpp:210)                */
  uint32_t tau;        /* --tau       [2]      (place only; unused by dist)       */
  double chisq;        /* --chisq     [2.706]                                     */
  double dist_max;     /* --dist-max  [NaN = unset]                               */
  uint32_t multi;      /* --multi     [1]                                         */
  uint32_t no_filter;  /* !--filter   [1 for dist] (src/krepp.cpp:635-644)        */
} kr_params;

KR_API void kr_params_default(kr_params*);

typedef struct kr_stream kr_stream;

/* max_reads / max_bases bound one submitted batch; device buffers are sized once.
 * max_records bounds the (read, strand, leaf) accumulators one batch may emit
 * (0 = default: max_reads * min(16, max(8, tree nodes + 1))); a batch that needs more
 * fails with KR_ERR_CAPACITY and can be resubmitted in smaller pieces. */
/* Kernels of all streams created on one kr_index run one batch after the other in submission order (a per-index
 * event chain); copies to and from the host overlap them.  Use two streams in turn to keep the GPU busy. */
KR_API int kr_stream_create(const kr_index*, const kr_params*, uint32_t max_reads, uint64_t max_bases,
                            uint64_t max_records, kr_stream** out);
KR_API void kr_stream_destroy(kr_stream*);

#define KR_BASES_HOST 0u
#define KR_BASES_DEVICE 1u /* bases/offsets already resident in this device's HBM */
#define KR_TAP_ACCS 2u     /* keep every (read,strand,leaf) histogram: rec_hist of the views, `place` */
#define KR_TAP_HITS 4u     /* record every table hit (debug; slow; the batch runs as one lane) */
#define KR_BASES_PINNED 8u /* host `bases` AND `offsets` are page-locked (hipHostMalloc / hipHostRegister, */
                           /* e.g. kr_host_alloc): copied to the device straight from the caller's       */
                           /* buffers, which must stay valid until the batch has been waited for         */
#define KR_ROWS_ONLY 16u   /* kr_batch_collect brings back only what the `dist` report needs         */
                           /* (read_off/cnt/na, rec_key/sel/d); rec_v, rec_chisq, rec_hist and        */
                           /* read_onmers of the host view are then NULL / undefined, and the kernels */
                           /* do not write rec_v at all (NULL in a device view too) unless the batch  */
                           /* filters (--filter) or taps.  The host view then holds the OUTPUT ROWS   */
                           /* only -- the records report_distances prints (src/query.cpp:158-196),    */
                           /* compacted on the device, 12 bytes a row across PCIe: nrecs == nrows,    */
                           /* every rec_sel is 1, read_off / read_cnt are the reads' row ranges (a    */
                           /* tiled batch still comes back as record slots with flags -- same fields, */
                           /* same meaning, rec_sel 0 where a record is not a row -- unless it is     */
                           /* submitted with KR_TILE_ROWS)                                            */
#define KR_ROWS_INDEXED 32u /* with KR_ROWS_ONLY: DIST leaves the device as an INDEX -- the likelihood    */
                           /* stage solves every distinct problem of a batch once (one in ~20 records), */
                           /* so a row is (rec_key, rec_dix), 8 bytes across PCIe instead of 12, and    */
                           /* the batch's distinct values come once: DIST of row i is                   */
                           /* dist_list[rec_dix[i]] (bit for bit what rec_d would hold); rec_d of the    */
                           /* host view is NULL then (a formatter may format each distinct value once). */
                           /* A hint: honoured for batches that run as one lane and are not tiled --     */
                           /* otherwise the view holds rec_d as without it (rec_dix == NULL says which). */
                           /* rec_dix != NULL exactly when it was honoured, and every rec_dix[i] of a row */
                           /* is then below ndist: a batch whose list positions outgrow the list (nearly  */
                           /* every record distinct, max_records set tightly) is run again by             */
                           /* kr_batch_wait / kr_batch_collect without the hint and comes back with      */
                           /* rec_d -- never an error the plain batch would not have raised.  A batch     */
                           /* without rows has ndist == 0.  A DEVICE view of an honoured batch holds      */
                           /* rec_dix per record slot (meaningful where rec_sel == 1), dist_list and      */
                           /* ndist as device data, rec_d == NULL.                                        */
#define KR_TILE_DEVICE 64u /* with KR_BASES_DEVICE (and for kr_batch_submit_fastq): long sequences of a batch that   */
                           /* is already in HBM are tiled too -- the tiled batch is laid out by kernels from the       */
                           /* caller's device bases / offsets (see "Long sequences" below).  The submit then WAITS    */
                           /* for a 24-byte summary of the layout before it returns.  Ignored for host input (which   */
                           /* is tiled anyway), with KR_TAP_HITS and while KR_NO_TILES is set                          */
#define KR_TILE_ROWS 128u  /* with KR_ROWS_ONLY: a batch that ends up TILED (a host batch with long sequences, or one tiled  */
                           /* with KR_TILE_DEVICE) leaves the device as compact rows too, exactly as an untiled rows batch: */
                           /* 12 bytes a row, a read's rows contiguous, nrecs == nrows, every rec_sel 1, read_off / read_cnt */
                           /* / read_na those of the CALLER's reads -- and a batch submitted with kr_batch_submit_text or   */
                           /* kr_batch_submit_fastq on a stream with text enabled has its report text written by the device */
                           /* (kr_batch_collect_text returns the bytes instead of KR_ERR_UNSUPPORTED).  Without the flag a   */
                           /* tiled batch comes back as record slots, holes of the tiles' own records included.  Opt-in;     */
                           /* ignored (never an error) with KR_TAP_ACCS / KR_TAP_HITS, while KR_NO_ROW_COMPACTION is set, and */
                           /* for a batch that does not end up tiled.  KR_ROWS_INDEXED stays not honoured for tiled batches  */
                           /* (rec_dix == NULL says so).  kr_batch_collect_device still shows record slots.                  */

/* Queue one batch: `bases` = concatenated ASCII sequences exactly as the FASTX
 * reader delivers them (QSeq::read_next_batch, src/rqseq.cpp:180-197),
 * offsets[nreads+1] = start of each read.  Asynchronous: host buffers must stay
 * valid until kr_batch_collect / kr_batch_wait returns.
 *
 * This replaces the reference's batching (src/rqseq.cpp:180-197 + the task loop src/krepp.cpp:360-387) by
 * pinned-host staging + hipMemcpyAsync: a HOST batch of >= 2 * 65,536 reads is cut into up to KR_LANES (env, default 2)
 * contiguous read ranges, each with its own HIP stream: the H2D copy, the kernels and (in kr_batch_collect) the
 * D2H copy of one range overlap with those of the other.  Results do not depend on the number of lanes.  Across
 * batches, two kr_streams used in turn overlap one batch's copies with the other's kernels (bench.py, the CLI).
 *
 * Long sequences (contigs, genomes): the reference scans a sequence serially (search_mers, src/query.cpp:40-94).  A HOST
 * batch that holds sequences of more than 1,024 k-mer positions is submitted as tiles of 128 positions (neighbours overlap by
 * k - 1 bases), which run on as many waves as there are tiles; the tiles' histograms are added per (reference, strand) and the
 * hdist_filt test is applied with the sequence's minimum, so the results are those of the serial scan (identical records, in
 * the same order).  A tile counts as a read against max_reads: the sequences whose tiles fit the stream are tiled, in order
 * (the others, and every sequence of a batch already in HBM or submitted with KR_TAP_HITS, are one wave's work as before); a
 * tiled batch whose tiles' records overflow the device buffers is run again untiled by kr_batch_wait / kr_batch_collect.  The
 * views always describe the caller's reads.
 *
 * A batch ALREADY IN HBM (KR_BASES_DEVICE) is tiled when it is submitted with KR_TILE_DEVICE: kernels (csrc/kr_dev_tiles.inc) count
 * the tiles, choose the sequences and lay the tiled batch out from the caller's device arrays -- the batch's bytes are read once
 * and written once, nothing crosses PCIe -- and the batch then runs exactly as a host batch's tiles do.  Two things differ from
 * the host's tiling.  The choice is a PREFIX rule: sequence r is tiled iff it is long and the tiles of the long sequences 0 .. r
 * together fit the stream (sum of nt - 1 <= max_reads - nreads); where the host, taking sequences greedily, may still tile a
 * shorter sequence behind one that did not fit, the device tiles none behind it.  This only matters when the room runs out, and
 * never for the results: tiled and untiled sequences give identical records.  And kr_batch_submit does not return before the
 * layout's summary (tiled reads, long sequences, bases: 24 bytes) has come back -- it waits for the kernels queued so far on the
 * stream's first lane, as kr_batch_submit_fastq waits for its summary; a batch without a long sequence is then queued as it is.
 * KR_TILE_MIN_POS is honoured; the caller's bases are read only inside [bases + offsets[0], bases + offsets[nreads]). */
KR_API int kr_batch_submit(kr_stream*, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads,
                           uint32_t flags);
KR_API int kr_batch_wait(kr_stream*);

/* One candidate row = one (read, leaf): what report_distances iterates over. */
typedef struct kr_result_view {
  uint32_t nreads;
  uint32_t nrecs;             /* (read, strand, leaf) accumulators that passed the       */
                              /* hdist_filt test (src/query.cpp:106,119)                  */
  const uint32_t* read_off;   /* [nreads] first record of the read                       */
  const uint32_t* read_cnt;   /* [nreads] number of records of the read                  */
  const uint32_t* read_onmers;/* [nreads] valid k-mer positions (src/query.cpp:66)       */
  const uint8_t* read_na;     /* [nreads] 1 = the read gets the "NA\tNaN" row             */
                              /* (src/query.cpp:173-176)                                 */
  const uint32_t* rec_key;    /* [nrecs]  (se << 1) | strand; ascending inside a read    */
  const uint8_t* rec_sel;     /* [nrecs]  1 = this record is an output row of `dist`     */
  const double* rec_d;        /* [nrecs]  d_llh                                          */
  const double* rec_v;        /* [nrecs]  v_llh                                          */
  const double* rec_chisq;    /* [nrecs]  chi-square vs the closest (filter mode), else NaN (NULL in a device view) */
  const uint32_t* rec_hist;   /* with KR_TAP_ACCS, else NULL: hist[x] of record i at      */
                              /* rec_hist[x * rec_hist_stride + i], x = 0..hdist_th       */
  uint64_t rec_hist_stride;
  uint64_t nrows;             /* number of rec_sel == 1                                  */
  const uint32_t* rec_dix;    /* KR_ROWS_INDEXED, honoured: [nrecs] index into dist_list (< ndist), rec_d == NULL; else NULL. */
                              /* Host view: per row.  Device view: per record slot, valid where rec_sel == 1                 */
  const double* dist_list;    /* [ndist] distinct d_llh values of the batch (unused positions hold anything); a device       */
                              /* pointer in a device view                                                                    */
  uint64_t ndist;             /* 0 for a batch without rows                                                                  */
} kr_result_view;

/* Waits for the batch and copies results to pinned host memory owned by the stream (lane by lane: a lane's
 * results travel while later lanes still compute).  Host view: records are compact, a read's records are
 * [read_off, read_off + read_cnt) in ascending key order; the order of the reads' record groups in the arrays
 * is not the read order (record slots are handed out to waves in chunks) and may differ from run to run. */
KR_API int kr_batch_collect(kr_stream*, kr_result_view* out);
/* As above but the arrays stay in HBM (device pointers); only counts are read back.  Device view: `nrecs` is
 * the extent of record slots handed out, unused slots (rec_key == 0) included; always go through read_off / read_cnt. */
KR_API int kr_batch_collect_device(kr_stream*, kr_result_view* out);
/* Bytes the last kr_batch_collect copied back over PCIe: rows or record slots, and the per-read arrays (measurement aid). */
KR_API int kr_debug_last_d2h_bytes(kr_stream*, uint64_t* bytes);
/* Tests: KR_ROWS_INDEXED -- `extent`: list positions the stream's last indexed launch handed out (holes included; of the first attempt
 * if the batch was then run again without the hint); `fallbacks`: batches of this stream run again so, so far.  Either may be NULL. */
KR_API int kr_debug_indexed_list(kr_stream*, uint64_t* extent, uint64_t* fallbacks);
/* Tests: crafted records through the production select and row kernels (tests/select_craft.py, tests/test_gpu_select_forms.py).
 * `kr_select_tables` is what the stages before the selection leave behind for one lane: the reads' record ranges, the records in key
 * order, and the values of the distinct likelihood problems, reached through the list (rec_rep = position) or through a direct place
 * (rec_rep = 0x80000000 | place, dd_direct[place] = position, dd_dv[place] = the value).  What the likelihood stage guarantees of them
 * is "The de-duplication's contract" in docs/design/05_likelihood_select_rows_text.md, tested through kr_debug_dedup below. */
typedef struct kr_select_tables {
  uint32_t nreads, nrecs;       /* reads; record slots in use (slots between two reads' ranges belong to nobody) */
  const uint32_t* rd_off;       /* [nreads] ascending, the ranges [rd_off, rd_off + rd_cnt) disjoint and within nrecs */
  const uint32_t* rd_cnt;       /* [nreads] */
  const uint32_t* rd_onmers;    /* [nreads] k-mers of the read */
  const uint32_t* rec_key;      /* [nrecs] se << 1 | strand, strictly ascending within a read, se below the index's node count */
  const uint32_t* rec_rep;      /* [nrecs] see above; 0xFFFFFFFF (a hole) only outside the reads' ranges */
  const uint64_t* rec_w0;       /* [nrecs] the packed problem (hdist_th 4 only), or 0: then rec_hist and rec_read describe the record */
  const uint32_t* rec_hist;     /* [nrecs][hdist_th + 1] row-major, or NULL if every record has a word */
  const uint32_t* rec_read;     /* [nrecs] the record's read, or NULL likewise */
  uint32_t nrep, ndirect;       /* list positions; direct places (0 unless the stream has a direct part: hdist_th 4) */
  const double* rep_dv;         /* [nrep][2] (d, v) */
  const uint32_t* dd_direct;    /* [ndirect] list position of the place, 0xFFFFFFFF for a place no record names */
  const double* dd_dv;          /* [ndirect][2] */
  uint32_t problems;            /* counters[kCtProblems]: the extent of the list the indexed rows' dist_list covers, at most nrep */
} kr_select_tables;
/* What the kernels wrote; every array is the caller's, any may be NULL.  The record arrays are read back behind the select kernel (the
 * indexed row kernel then reuses rec_d and rec_v), the rows behind the row kernels. */
typedef struct kr_select_result {
  uint8_t* rd_na;      /* [nreads] */
  uint32_t* rd_rcnt;   /* [nreads] rows modes; else as poisoned */
  uint32_t* rd_roff;   /* [nreads] likewise */
  uint8_t* rec_sel;    /* [nrecs] */
  double* rec_d;       /* [nrecs] */
  double* rec_v;       /* [nrecs] */
  double* rec_chisq;   /* [nrecs] */
  uint32_t* rec_rep;   /* [nrecs] behind the select kernel: indexed rows leave the resolved list position there */
  uint32_t* row_key;   /* [nrecs] rows modes: the first nrows entries are rows, the rest as the device left it */
  double* row_d;       /* [nrecs] plain rows */
  uint32_t* row_dix;   /* [nrecs] indexed rows */
  double* dist_list;   /* [problems] indexed rows */
  uint64_t nrows;      /* counters[kCtRows] in a rows mode, else 0 */
  uint32_t rows_mode, rows_indexed, keep_v; /* the lane's BatchOut fields as the submit path derives them from `flags` (the --filter kernel
                                             * writes rec_v whatever keep_v says) */
} kr_select_result;
/* Sets lane 0 of an idle one-lane stream up as kr_batch_submit(flags) would (flags: 0, KR_TAP_ACCS, KR_ROWS_ONLY, KR_ROWS_ONLY |
 * KR_ROWS_INDEXED), fills every output with 0xA5 bytes, uploads `in`, and runs the select kernel the stream's parameters call for
 * (form 0: as a batch would, KR_SELECT_LANE included; form 1: the wave-per-read kernel) and, in a rows mode, the row kernels.
 * KR_ERR_ARG for tables the kernels could not be given safely, KR_ERR_STATE for a stream with a batch in flight or several lanes. */
KR_API int kr_debug_select(kr_stream*, const kr_select_tables* in, uint32_t flags, uint32_t form, kr_select_result* out);
/* Tests (no device needed): the checks kr_debug_select makes of `in`, against limits given as numbers: reads and records the stream
 * holds, nodes of the index (rho entries), hdist_th, and the nodes the stream's direct part is laid out for (BatchOut::dd_nodes: tree nodes
 * + 1 at hdist_th 4, else 0; the library multiplies by its places per node).  KR_OK or KR_ERR_ARG. */
KR_API int kr_debug_select_check(const kr_select_tables* in, uint32_t max_reads, uint64_t max_records, uint32_t nnodes, uint32_t hdist_th,
                                 uint32_t direct_nodes);
/* Tests (no device needed): the constants the select and row kernels are compiled with: out8 = {most records of a read a lane walks
 * itself (kSelectLaneMax), lanes of the small and of the middle group (16, 32), lanes per read of the wave-per-read kernel
 * (KR_SELECT_GL), most records the big form keeps in registers (256), records per step of its second pass in memory (128), reads per
 * block of the row kernels (kRowBlock), reads the row kernel's workgroup takes per round (16)}. */
KR_API int kr_debug_select_layout(uint32_t* out8);
/* Tests: crafted records through the production likelihood de-duplication and minimisations (tests/dedup_craft.py,
 * tests/test_gpu_dedup_routes.py): the stage that leaves behind what kr_select_tables takes as given -- rec_rep, the list of distinct
 * problems, the direct places and their values; its contract is "The de-duplication's contract" in
 * docs/design/05_likelihood_select_rows_text.md.  `kr_dedup_tables` is what the accumulate stage leaves for one lane. */
typedef struct kr_dedup_tables {
  uint32_t nreads, nrecs;       /* reads; record slots handed out (counters[kCtRecSlots]) */
  const uint32_t* rd_off;       /* [nreads] ascending, the ranges [rd_off, rd_off + rd_cnt) disjoint and within nrecs */
  const uint32_t* rd_cnt;       /* [nreads] */
  const uint32_t* rd_onmers;    /* [nreads] k-mers of the read */
  const uint32_t* rec_key;      /* [nrecs] se << 1 | strand, se below the index's node count; 0 (a hole) at every slot outside the reads' ranges and nowhere else */
  const uint64_t* rec_w0;       /* [nrecs] the packed problem (hdist_th 4 only: counts in bits 0..39, the read's k-mers in 40..55, bit 63), or 0 */
  const uint32_t* rec_hist;     /* [nrecs][hdist_th + 1] row-major, read for records with rec_w0 == 0; NULL if there is none */
  const uint32_t* rec_read;     /* [nrecs] the record's read, likewise */
} kr_dedup_tables;
/* What the kernels wrote; every array is the caller's, any may be NULL.  rep_room, table_room and places_room are set by the caller: the
 * entries its rep_list / rep_dv, the slots its dd_table and the places its dd_direct / dd_dv hold; everything below them is set by the call. */
typedef struct kr_dedup_result {
  uint32_t* rec_rep;    /* [nrecs] list position, 0x80000000 | direct place, or 0xFFFFFFFF for a hole */
  uint32_t* rep_list;   /* [rep_room] the first rep_n entries: record index or 0xFFFFFFFF (hole) below `problems`, 0xA5 bytes beyond */
  double* rep_dv;       /* [rep_room][2] (d, v) of the listed problems; 0xA5 bytes at holes and beyond `problems` */
  uint32_t* dd_direct;  /* [places_room] list position of the place, 0xFFFFFFFF for a place no record names */
  double* dd_dv;        /* [places_room][2] the named places' values; 0xA5 bytes elsewhere */
  uint8_t* dd_oslot;    /* [256] k-mer count -> slot of the direct part, 0xFF none (untouched without a direct part) */
  uint64_t* dd_table;   /* [table_room][2] the first table_n slots of the lane's table: word, leaf | (position + 1) << 32; slots above `mask`
                         * are not this batch's (they hold what earlier batches left) */
  uint32_t rep_room, table_room, places_room;
  uint32_t rep_n, table_n;        /* entries copied: min(rep_room, rep_cap), min(table_room, dd_slots); of dd_direct / dd_dv: min(places_room, places) */
  uint32_t problems, err;         /* counters[kCtProblems], counters[kCtErr] */
  uint32_t rep_cap, places, dd_nodes, mask, dd_slots, dd_shift; /* the lane's list capacity, direct places (440 * dd_nodes), BatchOut::dd_nodes,
                                                                 * this batch's table mask, the table's slots, KR_DD_SHIFT as the stream read it */
} kr_dedup_result;
/* Sets lane 0 of an idle one-lane stream up as kr_batch_submit(0) would, fills every output of the stage with 0xA5 bytes (rec_rep, rep_list
 * and rep_dv up to the lane's capacity, dd_direct, dd_dv, dd_oslot; not the table), sets counters[kCtRecSlots] = nrecs and the other
 * counters 0, uploads `in` and queues the launches of a batch's likelihood stage.  KR_ERR_ARG for tables the kernels could not be given
 * safely, KR_ERR_STATE for a stream with a batch in flight or several lanes. */
KR_API int kr_debug_dedup(kr_stream*, const kr_dedup_tables* in, kr_dedup_result* out);
/* Tests (no device needed): the checks kr_debug_dedup makes of `in`, against limits given as numbers: reads and records the stream holds,
 * nodes of the index (rho entries) and hdist_th.  KR_OK, or KR_ERR_ARG with the reason in kr_last_error(): read ranges that overlap or
 * leave the records, a key beyond the nodes, a hole inside a read or a record outside every read, a packed word at another threshold,
 * without bit 63 or with a k-mer count that is not its read's, a record without word and histogram, a rec_read naming another read. */
KR_API int kr_debug_dedup_check(const kr_dedup_tables* in, uint32_t max_reads, uint64_t max_records, uint32_t nnodes, uint32_t hdist_th);
/* Tests (no device needed): the constants of the de-duplication kernels: out12 = {k-mer-count slots of the direct part (kDdOslots),
 * its classes (kDdClasses), most events of a direct problem (kDdMaxEvents), fewest table slots of a batch (kDdMinSlots), probe rounds
 * (kDdProbeRounds), list positions a wave takes at a time and at most (kRepChunk, kRepChunkMax), blocks of kr_dedup_kernel
 * (kDedupBlocks), reads per block of kr_dedup_oslot_kernel's grid (kDdOslotReads), low and high half of the word's hash multiplier
 * (kDdHashWord), the leaf's multiplier (kDdHashLeaf)}. */
KR_API int kr_debug_dedup_layout(uint32_t* out12);
/* Tests: path witnesses of the accumulate kernel for the batch last waited for, counted only by a stream created under
 * KR_DEBUG_SKIP=512 (0 otherwise): the first min(n, 21) into `out`, in this order -- finalize_events_fast: calls, returned false before
 * the compaction, compaction entered, returned false after it, finish_big_read, finished in one key batch, in several, key batches
 * beyond the first, fix_dup calls, fix_dup calls that moved the count; finalize_events: calls with events of the one-segment, the
 * two-segment and the merge instantiation, fused, sparse, planes in global scratch, key batches beyond the first, key table in global
 * scratch, returned false; process_read: reads set aside by the one-segment launch, reads done again with the plane tables. */
KR_API int kr_debug_acc_paths(kr_stream*, uint32_t* out, uint32_t n);
/* Tests (no device needed; the stream may be NULL): the event region of the accumulate instantiation for np = hdist_th + 1 planes and
 * reads of `segs` segments (1 or 2), or the merge instantiation (multi != 0): out8 = {events held in the LDS before a read's events
 * spill, words of the region, words per key of a batch of the straight-line epilogue, number of path witnesses, then for the stream
 * (0 if NULL) the events, passing-key table entries and keys a wave's global scratch holds, 0}. */
KR_API int kr_debug_acc_layout(const kr_stream*, uint32_t np, uint32_t segs, uint32_t multi, uint32_t* out8);
/* Tests (no device needed): the numbers of the scan shape chosen for a table of `slot_format` (0 packed: the shape follows log_g = 0,
 * 2, 3; 5..8 slotted; 9 filter slots), the constants the kernels are built with: out16 = {G lanes per probe, CPL 16-byte chunks per lane
 * and pass, PPS probes per pass, words per slot (0: packed), CAP entries a slot holds, step bits of a group before its hit chunks are
 * dealt out, probes a group lists at most, items staged per read before a flush, item slots a wave takes at a time, reads per visit to
 * a cursor, cursors, k-mer positions per segment, codes per line and per slot of format 9 (else 0), 1 if slotted, largest hdist_th
 * the scan of format 9 serves}. */
KR_API int kr_debug_scan_layout(uint32_t slot_format, uint32_t log_g, uint32_t* out16);
/* Tests: the scan of this stream: out4 = {1 if the pipelined slotted kernel is launched (formats 5..8; KR_SCAN_PIPE=0 when the stream is
 * made selects the one-group-at-a-time kernel), 1 if the filter-slot kernel is, item slots a lane's scan may use (KR_DEBUG_ITEM_CAP=n
 * when the stream is made lowers it), item slots the scan of the batch last waited for asked for}. */
KR_API int kr_debug_scan_stream(const kr_stream*, uint32_t* out4);
/* Tests: one number as `krepp place` rows print it (std::fixed, 5 decimals; `out` holds 80 bytes); returns its length. */
KR_API int kr_debug_place_fixed5(double v, char* out);

/* Debug taps (parity tests).  Hits: one entry per table entry with hd <= hdist_th. */
typedef struct kr_hit {
  uint32_t read;
  uint32_t kpos;    /* k-mer start index in the read                               */
  uint32_t strand;
  uint32_t lib;
  uint64_t cmer_index;
  uint32_t hd;
  uint32_t se;
} kr_hit;
KR_API int kr_batch_hits(kr_stream*, const kr_hit** hits, uint64_t* nhits);
typedef struct kr_readtap {
  uint32_t hdist_filt[2]; /* per-strand min hd over kept entries, 0xFFFFFFFF = none */
} kr_readtap;
KR_API int kr_batch_readtaps(kr_stream*, const kr_readtap** taps);

/* Experiments (the scan kernel's launch-time levels): give one group of a stream's device buffers a new
 * address -- 0: item list, 1: per-read arrays, 2: counters and cursors, 3: records and de-duplication table -- or its kernels a
 * new HIP stream (4).  Between batches only; results are unaffected. */
KR_API int kr_debug_stream_move(kr_stream*, int which);
/* ... and where they are: item list, counters, cursors, rd_off, rd_it_off, rd_filt, rec_key, de-duplication table. */
KR_API int kr_debug_stream_addrs(kr_stream*, uint64_t* out8);

/* Item-list placement: a stream that is given batches of a million reads or more allocates its item list
 * (the scan kernel's output) up to KR_ITEM_PLACEMENT_TRIALS more times (environment, default 3, 0 = never) during its first
 * batches -- one spare list at a time -- and keeps the allocation the scan kernel ran fastest on; the kernel's launch time depends
 * on the physical pages behind the list (40.5 against 46.5 ms per 8 M reads), which only a new allocation changes.  Results are
 * unaffected.  This call reports what the stream did: allocations tried, how many of them replaced the one before, and the scan
 * time per read on the list it kept. */
KR_API int kr_debug_item_placement(kr_stream*, uint32_t* tried, uint32_t* kept, double* best_ns_per_read);

/* Front-end tap: rix / enc32 / residue test for every (k-mer, strand) of one batch,
 * laid out [read][kpos][strand] with `stride` = max k-mers per read; valid==0 marks
 * positions whose window holds a non-ACGT byte or runs past the read. */
KR_API int kr_debug_front_end(const kr_index*, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads,
                              uint32_t stride, uint32_t* rix, uint32_t* enc32, uint8_t* valid, uint8_t* pass);

/* The host pass of kr_index_upload over a library's colour table (no device needed): the tagged form of every colour id
 * (class in the top two bits: 0 drop, 1 leaf rank, 2 walk through se_to_pse, 3 flat), the se_to_pse table as the device holds it
 * ({part, part} tagged, or for a flat colour {base | list flag << 31, count}) and the leaf lists.  node_kind[se], se <= tree_nnodes:
 * 0 null, 1 leaf, 2 internal (as in kr_index_view).  *nlist: in = capacity of lists_out in entries, out = entries needed.
 * Replaces the per-hit walk of src/query.cpp:369-387 for the colours whose leaves can be named at upload. */
KR_API int kr_debug_colour_classes(const uint32_t* pse_pairs /*[2*nsubsets]*/, uint32_t nsubsets, const uint8_t* node_kind, uint32_t tree_nnodes,
                                   uint32_t* cls_out /*[nsubsets]*/, uint32_t* pse_out /*[2*nsubsets]*/, uint32_t* lists_out, uint64_t* nlist);

/* Likelihood + minimiser on their own (device): one problem per element. */
KR_API int kr_debug_brent(const kr_index*, uint32_t hdist_th, uint32_t n, const uint32_t* hist /*[n*(th+1)]*/,
                          const uint32_t* onmers, const double* rho, double* d_out, double* v_out);

/* The prefix-sum helpers of the compacting stages (kr_dev_prefix.inc) on plain numbers, run as those stages run them: sums per
 * block of `block` values (64 or 1024), one workgroup's scan of the block sums, the exclusive scan inside every block; sums of
 * `width` bytes (4 or 8; with 4 the caller keeps the total below 2^32).  prefix[i] = values[0] + ... + values[i - 1], *total = the
 * sum of all n.  n = 0: *total = 0 and nothing is launched.  Runs on the calling thread's current device. */
KR_API int kr_debug_prefix(const uint32_t* values, uint32_t n, uint32_t block, uint32_t width, uint64_t* prefix /*[n]*/, uint64_t* total);

/* Likelihood kernel on arbitrary problems (the per-edge likelihoods of `krepp place`, whose
 * histograms are fractional: Minfo::add, src/query.hpp:139-152).  One problem per element:
 * hist[n*(th+1)] (doubles), uc[n] = mismatch_count, rho[n].  mode 0: Brent minimisation
 * (Minfo::optimize_likelihood, src/query.cpp:426-433) -> d_out, v_out.  mode 1: evaluate f at
 * d_in[n] -> v_out (Minfo::likelihood_ratio's f(d), src/query.cpp:420-424). */
KR_API int kr_llh_batch(const kr_index*, uint32_t hdist_th, uint32_t mode, uint64_t n, const double* hist, const double* uc,
                        const double* rho, const double* d_in, double* d_out, double* v_out);
/* f_{problem pidx[i]}(d_in[i]), i < n: many evaluations of few problems (hist [nprob * (th + 1)], uc, rho [nprob]) --
 * the chi-square tests of `place` (src/query.cpp:276, :420-424): every candidate of a read against its closest leaf. */
KR_API int kr_llh_eval_indexed(const kr_index*, uint32_t th, uint64_t nprob, const double* hist, const double* uc, const double* rho,
                               uint64_t n, const uint32_t* pidx, const double* d_in, double* v_out);

/* Kernel timing of the last collected batch (HIP events on the stream's own stream). */
typedef struct kr_timing {
  float ms_total;    /* first kernel start -> last kernel end                        */
  float ms_scan;     /* kr_scan_kernel: front end + table scan (the dominant kernel) */
  float ms_acc;      /* kr_acc_kernel: colour expansion + histograms + records       */
  float ms_llh;      /* likelihood + selection kernels                               */
  float ms_h2d;      /* host->device copies (0 with KR_BASES_DEVICE)                 */
  uint32_t overflow_reads; /* reads that took the global-memory accumulator path     */
  uint32_t stack_spills;   /* times a colour-expansion stack outgrew the LDS (large clades) */
  uint32_t lanes;          /* read ranges the batch was cut into: with one, ms_scan/acc/llh are the kernels' own  */
                           /* durations; with several they are sums over lanes that share the chip (> ms_total)   */
} kr_timing;
KR_API int kr_batch_timing(kr_stream*, kr_timing* out);

/* ------------------------------------------------------------------------- */
/* Host helpers mirroring the reference's reader and writer.                    */
/* ------------------------------------------------------------------------- */
/* QSeq (src/rqseq.cpp:146-203): gz/FASTA/FASTQ batches of >= 76,800 bases.  Plain (uncompressed)   */
/* regular files of >= 32 MB are cut at record starts and parsed by a thread pool (KR_FASTX_THREADS,   */
/* default min(8, cores/2); 0 = off): a batch is then one chunk of about 2 * min_bases bytes of input. */
/* Block-gzipped files (BGZF: independent members with a "BC" extra field) are inflated member by       */
/* member on the same threads (CRC-checked; a damaged member is KR_ERR_IO); ordinary gzip is one stream  */
/* and is inflated by zlib in the calling thread.  (The members can be inflated on the device instead:  */
/* kr_batch_submit_bgzf, below.)                                                                         */
/* Records, names and order are those of the sequential reader in every case.                          */
typedef struct kr_fastx kr_fastx;
typedef struct kr_fastx_batch {
  const uint8_t* bases;
  const uint64_t* offsets;     /* [nreads+1] */
  const char* const* names;    /* [nreads]   NUL-terminated, back to back in one buffer, in order */
  uint32_t nreads;
  uint32_t more;               /* 0 once the input is exhausted                    */
} kr_fastx_batch;
KR_API int kr_fastx_open(const char* path, kr_fastx** out);
/* The sequential reader (kseq's grammar, no thread pool) on a plain file from byte `offset`, which must be a record start: one byte
 * past the end of a record, or 0.  kseq's state there is "look for the next '>' / '@'", so the records read from `offset` are the
 * tail of the records read from the start of the file, byte for byte.  gzip input: KR_ERR_UNSUPPORTED (no byte offsets into it). */
KR_API int kr_fastx_open_at(const char* path, uint64_t offset, kr_fastx** out);
KR_API int kr_fastx_next(kr_fastx*, uint64_t min_bases, kr_fastx_batch* out);
/* The batch kr_fastx_next just returned changes hands (what QSeq gives IBatch by swap, src/query.cpp:32-33): the kr_fastx_batch's
 * pointers stay valid, nothing is copied, until kr_fastx_release hands the buffers back for reuse -- from any thread, before
 * kr_fastx_close.  For consumers that keep several batches in flight (the CLI's workers). */
typedef struct kr_fastx_held kr_fastx_held;
KR_API int kr_fastx_detach(kr_fastx*, kr_fastx_held** out);
KR_API void kr_fastx_release(kr_fastx*, kr_fastx_held*);
KR_API uint64_t kr_fastx_parallel_chunks(const kr_fastx*); /* chunks taken from the thread pool so far */
/* ordinary gzip input (csrc/kr_pgz.inc): chunks handed out with their records parsed by the pool / chunks whose speculative start
 * the verified stream did not pass through (their range was inflated by the reader) / gaps closed by the reader */
KR_API void kr_fastx_pgz_stats(const kr_fastx*, uint64_t* parsed, uint64_t* discarded, uint64_t* gaps);
KR_API void kr_fastx_close(kr_fastx*);

/* report_distances text (src/query.cpp:158-196; DISTANCE_FIELDS src/query.hpp:210;
 * std::fixed, precision 5 src/query.cpp:152-153).  Appends to a malloc'ed buffer. */
KR_API int kr_format_dist(const kr_host_index*, const kr_result_view*, const char* const* names, char** text,
                          uint64_t* len);
/* `krepp seek` rows `SEQ_ID\tDIST` / `SEQ_ID\tNaN` (SBatch::seek_sequences, src/seek.cpp:22-56) from a batch
 * on a sketch index; stream parameters multi = 1, no_filter = 1, dist_max unset. */
KR_API int kr_format_seek(const kr_host_index*, const kr_index*, const kr_result_view*, uint32_t hdist_th,
                          const char* const* names, char** text, uint64_t* len);
/* The same rows as TEXT written by the GPU (csrc/kr_dev_text.inc): IBatch::report_distances (src/query.cpp:158-196) ran inside the
 * reference's parallel batch task; kr_format_dist runs on host threads at ~100 M rows/s, 45 times under the kernels on a 1000-genome
 * index (33 rows per read).  A stream with text enabled formats its rows-only batches on the device -- SEQ_ID, reference name,
 * "%.5f" of DIST with printf's own rounding (round-half-even of the exact binary value), "SEQ_ID\tNA\tNaN" for a read without rows --
 * into a text buffer in HBM that is copied back as bytes: the host only write()s them, in batch order.
 *   kr_stream_text_enable   once per stream: uploads the index's node names (once per kr_index) and sizes the stream's id and text
 *                           buffers (max_text_bytes of page-locked host memory and as much HBM; max_id_bytes for a batch's ids)
 *   kr_batch_submit_text    kr_batch_submit(flags | KR_ROWS_ONLY) + the reads' ids: `ids` holds them back to back in read order,
 *                           id r = ids[id_off[r] .. id_off[r+1] - id_sep) (id_sep = 1 for NUL-terminated names, as kr_fastx_batch
 *                           delivers them); ids and id_off may be pageable, they are staged before the call returns
 *   kr_batch_collect_text   waits, copies the text back; *text points into the stream's page-locked buffer and stays valid until the
 *                           next submit on this stream.  KR_ERR_CAPACITY: more text (or ids) than the buffers hold -- resubmit in
 *                           smaller pieces; KR_ERR_UNSUPPORTED: the batch could not be formatted on the device (it was tiled -- long
 *                           sequences -- and submitted without KR_TILE_ROWS; or a DIST outside [0, 1000)): kr_batch_collect +
 *                           kr_format_dist still serve it, no resubmit.
 * Byte-identical to kr_format_dist (tests/test_gpu_text.py). */
KR_API int kr_stream_text_enable(kr_stream*, const kr_host_index*, uint64_t max_text_bytes, uint64_t max_id_bytes);
KR_API int kr_batch_submit_text(kr_stream*, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads, uint32_t flags,
                                const char* ids, const uint32_t* id_off, uint32_t id_sep);
KR_API int kr_batch_collect_text(kr_stream*, const char** text, uint64_t* len);
KR_API uint32_t kr_debug_fixed5(double v, char* out); /* tests: the device formatter's "%.5f" (0: outside [0, 1000)) */
KR_API void kr_free(void*);
/* Page-locked host memory for read batches (KR_BASES_PINNED): what a reader fills instead of a std::string. */
KR_API void* kr_host_alloc(uint64_t bytes);
KR_API void kr_host_free(void*);

/* FASTQ records found on the device (csrc/kr_dev_fastq.inc): a batch given as the raw bytes of a plain FASTQ file.  The chunk is
 * copied to HBM, its newlines are found and every record r (lines 4r .. 4r+3) is checked; the accepted prefix's bases, offsets and
 * ids are written where kr_batch_submit / kr_batch_submit_text put them, and the batch runs as they run it.  A record is accepted
 * ("device-clean") iff the host reader's four-line fast path takes it AND its quality line is exactly as long as its sequence line:
 * '@' header, sequence bytes 33..126 other than '>' '+' '@', a line starting with '+', quality bytes 33..127.  Its name runs from
 * after the '@' to the first C-locale isspace byte.  The accepted records are then those the sequential reader gives for the same
 * bytes, with the same names and sequences; the prefix ends at the first record that is not accepted (`status`):
 *   KR_FASTQ_NOT_CLEAN    anything else (FASTA, CRLF, wrapped lines, odd quality ...): the host reader continues at `consumed`
 *                         (FASTA has an entry point of its own: kr_batch_submit_fasta, below)
 *   KR_FASTQ_INCOMPLETE   bytes behind the last complete record: a record cut by the end of the chunk, or a last line without '\n'
 *   KR_FASTQ_LONG         more k-mer positions than the stream tiles a sequence from (KR_TILE_MIN_POS): the host path tiles it
 *                         (never raised with KR_TILE_DEVICE in `flags`: the record is accepted like any other, bounded by max_reads,
 *                         max_bases and the id buffer, and the accepted prefix is submitted with KR_BASES_DEVICE | KR_TILE_DEVICE.
 *                         A batch that ends up tiled is formatted on the device only with KR_TILE_ROWS in `flags` as well;
 *                         without it kr_batch_collect_text gives KR_ERR_UNSUPPORTED, and kr_batch_collect + kr_format_dist
 *                         with kr_batch_fastq_names serve it)
 *   KR_FASTQ_CAPACITY     past max_reads, max_bases or the id buffer: submit again from `consumed` (nreads 0: the record never fits)
 *   kr_stream_fastq_enable  once per stream: device buffers for chunks of up to max_raw_bytes (< 4 GB: positions are 32-bit)
 *   kr_batch_submit_fastq   `raw` is page-locked (kr_host_alloc), starts at a record start and stays valid until the batch has been
 *                           waited for.  Copies it, runs the parse kernels on the stream (beside the previous batch's kernels of other
 *                           streams), waits for the 64-byte summary only, and with nreads > 0 queues the batch like kr_batch_submit
 *                           with KR_BASES_DEVICE -- or, on a stream with text enabled and no tap flags, like kr_batch_submit_text with
 *                           id_sep 0 (the ids are already on the device).  nreads == 0: nothing is queued.  at_eof: `raw` ends where
 *                           the file does (recorded in the summary; INCOMPLETE there leaves the file's last record to the host reader)
 *   kr_batch_fastq_names    the accepted records' names as (position in `raw`, length), for the host formatters (kr_format_dist, the
 *                           KR_ERR_UNSUPPORTED path of kr_batch_collect_text); valid until the next submit on the stream */
#define KR_FASTQ_OK 0u
#define KR_FASTQ_NOT_CLEAN 1u
#define KR_FASTQ_INCOMPLETE 2u
#define KR_FASTQ_LONG 3u
#define KR_FASTQ_CAPACITY 4u
typedef struct kr_fastq_parse { /* 64 bytes, written by the device */
  uint64_t consumed;  /* the byte just past the last accepted record (0: none)                */
  uint64_t nbases;    /* bases of the accepted records                                        */
  uint64_t id_bytes;  /* name bytes of the accepted records (0 without text)                  */
  uint64_t newlines;  /* '\n' bytes in the chunk                                              */
  uint32_t nreads;    /* accepted records                                                     */
  uint32_t status;    /* KR_FASTQ_*                                                           */
  uint32_t rejected;  /* index of the first record not accepted (== nreads)                   */
  uint32_t at_eof;    /* the caller's at_eof                                                  */
  uint32_t reserved[4];
} kr_fastq_parse;
KR_API int kr_stream_fastq_enable(kr_stream*, uint64_t max_raw_bytes);
KR_API int kr_batch_submit_fastq(kr_stream*, const uint8_t* raw, uint64_t nbytes, uint32_t flags, uint32_t at_eof, kr_fastq_parse* out);
KR_API int kr_batch_fastq_names(kr_stream*, const uint64_t** name_pos, const uint32_t** name_len);
/* tests: the last kr_batch_submit_fastq's accepted bases [nbases] and offsets [nreads + 1] as the device wrote them */
KR_API int kr_debug_fastq_batch(kr_stream*, uint8_t* bases, uint64_t* offsets);
/* measurements: the device time (ms) of the record finder's kernels in the stream's last kr_batch_submit_fastq / _fasta.  The first
 * call makes the events and gives -1; every parse behind it is measured (two event records a submit) */
KR_API int kr_debug_fastq_parse_ms(kr_stream*, float* ms);

/* FASTA records found on the device (csrc/kr_dev_fasta.inc): a batch given as the raw bytes of a plain FASTA file -- contigs,
 * assemblies, genomes: wrapped at any width, LF or CRLF, or one line of megabases per record.  The stream is the one
 * kr_stream_fastq_enable prepared, `raw` and `flags` are bound as for kr_batch_submit_fastq (page-locked, below 4 GB, at most
 * max_raw_bytes, no KR_BASES_* flags), the summary is the same kr_fastq_parse (`newlines`: the chunk's '\n' bytes, `at_eof`: the
 * caller's `closed`), the accepted prefix is queued exactly as kr_batch_submit_fastq queues its own (KR_TILE_DEVICE and
 * KR_TILE_ROWS are honoured the same way, nreads == 0 queues nothing), and kr_batch_fastq_names / kr_debug_fastq_batch serve it
 * afterwards.  Every pass over the chunk's bodies is parallel over its bytes, never over a record's length (only a header is
 * walked by one wave), so that a 4 MB record should cost about what 4 MB of short records cost (measured, 64 MB of each:
 * docs/design/08, "FASTA records on the device").  The device buffers only FASTA needs are made by a stream's first kr_batch_submit_fasta (sized from
 * max_raw_bytes and max_reads); kr_batch_submit_fastq still answers NOT_CLEAN for FASTA.
 * The grammar ("device-clean FASTA"), a subset of what the sequential reader takes (character-wise: src/kseq.h:177-219), on which
 * both give the same names and sequences:
 *   record start   a '>' at byte 0 of the chunk or directly behind a '\n'.  The chunk must begin with one (else NOT_CLEAN, nreads 0)
 *   header         from the record start through the next '\n' (not in the chunk: the record is INCOMPLETE)
 *   name           from behind the '>' to the first C-locale isspace byte of the header; may be empty; a NUL byte in it makes the
 *                  record NOT_CLEAN (the host's names are C strings).  Other header bytes are free: comments may hold > + @, bytes >= 128
 *   body           from behind the header's '\n' to the next record start, or to the end of the chunk
 *   sequence       the body's bytes 33..126, in order; bytes below 33 and byte 127 are dropped ('\n', '\r', blanks, tabs, blank lines)
 *   not clean      a body that holds '+', '@', a '>' that is no record start, or a byte >= 128 (the reader ends a record at the first
 *                  three anywhere, and takes 0xFF for the end of the file): that record ends the accepted prefix with NOT_CLEAN
 *   last record    a FASTA record does not say where it ends, so the caller does: closed != 0 -- the chunk ends where the file does, or
 *                  at a byte where the caller has seen the next record start -- makes the chunk's last record complete, with or
 *                  without a final '\n'; with closed == 0 the last record is never accepted (INCOMPLETE)
 *   consumed       the position of the first record start that was not accepted, or nbytes: kr_fastx_open_at(path, chunk_offset +
 *                  consumed) yields exactly the remaining records.  status == KR_FASTQ_OK iff consumed == nbytes; rejected == nreads
 *   KR_FASTQ_LONG / KR_FASTQ_CAPACITY   as for FASTQ (LONG is never raised with KR_TILE_DEVICE; nreads 0: the record never fits)
 * kr_fasta_chunk_cut (no device): the position of the last record start in buf[1 .. n), 0 when there is none -- where a reader of
 * raw bytes ends a chunk that it submits with closed = 1 (`krepp dist --gpu-parse`).
 * kr_fastq_chunk_cut (no device): where the same reader ends a chunk of FASTQ -- the last line start c in the chunk's last MiB,
 * behind the first newline there, with buf[c] == '@', the line after next starting with '+', both lines between them complete and
 * that '+' inside buf[0 .. n); 0 when there is none (the chunk is submitted whole and its last record stops INCOMPLETE). */
KR_API int kr_batch_submit_fasta(kr_stream*, const uint8_t* raw, uint64_t nbytes, uint32_t flags, uint32_t closed, kr_fastq_parse* out);
KR_API uint64_t kr_fasta_chunk_cut(const uint8_t* buf, uint64_t n);
KR_API uint64_t kr_fastq_chunk_cut(const uint8_t* buf, uint64_t n);
/* kr_fastq_pair_cut (no device): the cut of a reader of PAIRED four-line FASTQ (`krepp seek --query2 / --interleaved`).  a and b each
 * begin at a record start; *nrec is the largest n <= max_records such that both hold 4n complete lines, *cut_a / *cut_b the byte
 * behind the 4n-th '\n' of each (0 when n is 0).  b == NULL (nb ignored, cut_b may be NULL): one buffer with the mates as
 * neighbours -- the largest EVEN n.  Only newlines are counted: whether the records are clean is the device record finder's to say.
 * KR_ERR_ARG: a, cut_a or nrec is NULL, or b without cut_b. */
KR_API int kr_fastq_pair_cut(const uint8_t* a, uint64_t na, const uint8_t* b, uint64_t nb, uint32_t max_records, uint64_t* cut_a, uint64_t* cut_b, uint32_t* nrec);

/* ---- block-gzipped bytes inflated on the device (csrc/kr_inflate.h, csrc/kr_dev_bgzf.inc; docs/design/08 "BGZF on the device") ----
 * A BGZF file is a run of independent gzip members of at most 64 KB of inflated bytes; each announces its compressed size ("BC"
 * extra field) and its inflated size (ISIZE).  kr_batch_submit_bgzf takes WHOLE members, inflates them on the device -- one wave
 * per member, CRC-32 checked there -- into the buffer the record finders read, and is from there on kr_batch_submit_fastq
 * (fasta == 0) or kr_batch_submit_fasta (fasta != 0) for those bytes.
 *   kr_stream_bgzf_enable   once per stream, after kr_stream_fastq_enable (else KR_ERR_STATE; twice: KR_ERR_STATE): device buffers for
 *                           up to max_comp_bytes (< 4 GB) of compressed bytes, a table of max_comp_bytes / 28 + 1 members, their
 *                           statuses and two 64 KB scratch windows
 *   kr_batch_submit_bgzf    `comp` is page-locked and holds whole members only, U inflated bytes in all.  The chunk is bytes
 *                           [skip, skip + nbytes) of them: skip lies inside the first member, skip + nbytes <= U, nbytes <=
 *                           max_raw_bytes, and only the first and the last member may reach outside the chunk (KR_ERR_ARG).
 *                           raw_out (page-locked, [nbytes], may be NULL) receives the chunk's bytes; `out`, kr_batch_fastq_names
 *                           (positions in raw_out), kr_debug_fastq_batch, kr_place_stream_parsed(raw = raw_out) and the flags are
 *                           those of a raw-bytes submit of raw_out[0 .. nbytes).  After KR_FASTQ_CAPACITY the caller goes on
 *                           with kr_batch_submit_fastq(raw_out + consumed, ...).  KR_ERR_FORMAT: bytes that are no whole BGZF
 *                           member, ISIZE above 65,536, a member the decoder rejects, a wrong CRC or length -- the message names the
 *                           member's offset in `comp` and the rule; nothing is queued and the stream serves the next submit.
 *   kr_debug_bgzf_inflate   (tests) the inflate kernel alone: all U bytes of comp's members into out[0 .. cap), U <= max_raw_bytes
 *   kr_debug_bgzf_inflate_host  the same members through the decoder's host instantiation: no device, the same codes and messages
 *   kr_debug_bgzf_ms        (measurements) device time of the inflate kernel of the stream's last chunk; as kr_debug_fastq_parse_ms
 * No device:
 *   kr_bgzf_member_size     the size of the BGZF member that starts at h[0 .. avail), 0 when these bytes are not one
 *   kr_bgzf_walk            the whole, well-formed members at the front of buf whose inflated sizes stay within max_inflated (always
 *                           one when one is complete): their number, compressed and inflated bytes
 *   kr_bgzf_chunk_cut       the last record start of the chunk that is bytes [skip, U) of buf's members, as the member's offset in buf
 *                           and the byte inside it (the trailing members are inflated with zlib, the last two first, then up to
 *                           1 MiB, and cut by kr_fastq_chunk_cut / kr_fasta_chunk_cut); returns the cut's position in the chunk, 0
 *                           when there is none
 *   kr_fastx_open_at_bgzf   the host reader from byte uoff of the member at file offset member_off, a record start (kr_fastx_open_at
 *                           for a block-gzipped file); bytes at member_off that are no BGZF member are read as ordinary gzip */
KR_API int kr_stream_bgzf_enable(kr_stream*, uint64_t max_comp_bytes);
KR_API int kr_batch_submit_bgzf(kr_stream*, const uint8_t* comp, uint64_t ncomp, uint32_t skip, uint64_t nbytes, uint8_t* raw_out,
                                uint32_t flags, uint32_t fasta, uint32_t at_eof_or_closed, kr_fastq_parse* out);
KR_API int kr_debug_bgzf_inflate(kr_stream*, const uint8_t* comp, uint64_t ncomp, uint8_t* out, uint64_t cap, uint64_t* len);
KR_API int kr_debug_bgzf_inflate_host(const uint8_t* comp, uint64_t ncomp, uint8_t* out, uint64_t cap, uint64_t* len);
KR_API int kr_debug_bgzf_ms(kr_stream*, float* ms);
KR_API uint32_t kr_bgzf_member_size(const uint8_t* h, uint64_t avail);
KR_API int kr_bgzf_walk(const uint8_t* buf, uint64_t n, uint64_t max_inflated, uint32_t* nmembers, uint64_t* comp_bytes, uint64_t* inflated);
KR_API uint64_t kr_bgzf_chunk_cut(const uint8_t* buf, uint64_t comp_bytes, uint32_t skip, uint32_t fasta, uint64_t* member_off, uint32_t* uoff);
KR_API int kr_fastx_open_at_bgzf(const char* path, uint64_t member_off, uint32_t uoff, kr_fastx** out);

/* ---- ordinary gzip inflated on the device (csrc/kr_inflate_sym.h, csrc/kr_gzip_super.h, csrc/kr_dev_gzip.inc; docs/design/08
 * "Ordinary gzip on the device") ----
 * An ordinary gzip member is ONE dependent deflate stream.  The inflater takes a SUPER-CHUNK of at most max_comp_bytes compressed
 * bytes from where the verified stream stands, cuts it into sub-chunks of sub_bytes (one wave each) and runs four kernels: search (the
 * first dynamic block start in every sub-chunk), decode (symbolically, against an unknown 32 KB window, into a slot of ratio_cap
 * symbols per compressed byte), chain (the sub-chunks the stream passes through, and the window behind each), resolve (symbols to
 * bytes, CRC-32).  The host compares every member's CRC-32 and length with its trailer, as gzread would.  It is independent of
 * kr_stream: its own HIP stream on one device, buffers sized at creation (about 3 * ratio_cap * max_comp_bytes device bytes).
 *   kr_gzdev_open      a regular file that starts with a gzip member.  sub_bytes >= 64, 1 <= ratio_cap <= 1024, max_comp_bytes >=
 *                      sub_bytes, below 512 MB, ratio_cap * max_comp_bytes < 2^31 (else KR_ERR_ARG); keep_points >= 4 (fewer: 4)
 *   kr_gzdev_read      the next inflated bytes in file order into dst[0 .. cap) (page-locked for the copy to be asynchronous); *n == 0:
 *                      the end.  KR_ERR_IO ("damaged gzip file PATH: ... (at compressed offset N)") for a broken stream, a wrong CRC-32
 *                      or length -- AFTER the bytes in front of the damage were handed out, as on every host path.  Bytes behind the
 *                      last member that are no gzip member are ignored
 *   kr_gzdev_point     the restart point at or in front of inflated_off among the starts of the last keep_points super-chunks
 *                      (KR_ERR_ARG: none is kept that far back)
 *   kr_gzdev_counters  c[11] = super-chunks, sub-chunks linked, sub-chunks without a start, sub-chunks dropped, host ranges (stretches
 *                      zlib inflated because the first sub-chunk could not finish: a ratio above ratio_cap, a block larger than the
 *                      super-chunk; inflated and handed out in pieces of about 64 MB, whatever they inflate to), redone bytes
 *                      (compressed bytes that super-chunks took in behind their verified end -- a member's end, an overflow, a start
 *                      nobody linked to -- and the next super-chunk copies, searches and decodes again: a file of many small members
 *                      concatenated pays max_comp_bytes of work per member, and this counter says so), device time (us, by events) of
 *                      the search, decode, chain and resolve kernels, time (us) of the copies
 *   kr_fastx_open_at_gzip   the host reader so that it yields exactly the records from inflated_off on: zlib primed at the point
 *                      (NULL: from the file's start), the members' trailers checked from the point's CRC state
 *   kr_debug_gzdev_inflate       (tests) a whole gzip buffer through the kernels: its bytes, the rows of every super-chunk's sub-chunks one
 *                      after the other (start bit S or 0xFFFFFFFF, end bit, status 0 idle / 1 linked / 2 member end / 3 input end /
 *                      4 overflow / 5 bad, link, symbols, CRC-32 of a chain chunk), counters[6] as the first six above
 *   kr_debug_gzdev_inflate_host  the same pipeline through the stages' serial instantiation: no device; the same bytes, rows, counters,
 *                      codes and messages
 *   kr_debug_gzdev_point_host    (tests) the restart point the serial twin keeps at or in front of inflated_off once it has read that far */
typedef struct kr_gzdev kr_gzdev;
typedef struct kr_gzip_point {
  uint64_t bit;          /* compressed bit position in the file */
  uint64_t inflated_off; /* of the first byte inflated from there */
  uint64_t member_len;   /* the member's length in front of the point */
  uint32_t member_crc;   /* ... and its CRC-32 */
  uint32_t window_len;   /* bytes of window[] in use: its LAST window_len bytes */
  uint8_t window[32768];
} kr_gzip_point;
KR_API int kr_gzdev_open(const char* path, int device, uint64_t max_comp_bytes, uint32_t sub_bytes, uint32_t ratio_cap, uint32_t keep_points, kr_gzdev** out);
KR_API void kr_gzdev_close(kr_gzdev*);
KR_API int kr_gzdev_read(kr_gzdev*, uint8_t* dst, uint64_t cap, uint64_t* n);
KR_API int kr_gzdev_point(const kr_gzdev*, uint64_t inflated_off, kr_gzip_point* out);
KR_API int kr_gzdev_counters(const kr_gzdev*, uint64_t* c11);
KR_API int kr_fastx_open_at_gzip(const char* path, uint64_t inflated_off, const kr_gzip_point* from, kr_fastx** out);
KR_API int kr_debug_gzdev_inflate(int device, const uint8_t* comp, uint64_t n, uint32_t sub_bytes, uint32_t ratio_cap, uint64_t max_comp_bytes, uint8_t* out,
                                  uint64_t cap, uint64_t* len, uint64_t tab_cap, uint32_t* S, uint32_t* end, uint32_t* status, uint32_t* link,
                                  uint32_t* length, uint32_t* crc, uint64_t* ntab, uint64_t* counters);
KR_API int kr_debug_gzdev_point_host(const uint8_t* comp, uint64_t n, uint32_t sub_bytes, uint32_t ratio_cap, uint64_t max_comp_bytes, uint64_t inflated_off,
                                     kr_gzip_point* out);
KR_API int kr_debug_gzdev_inflate_host(const uint8_t* comp, uint64_t n, uint32_t sub_bytes, uint32_t ratio_cap, uint64_t max_comp_bytes, uint8_t* out,
                                       uint64_t cap, uint64_t* len, uint64_t tab_cap, uint32_t* S, uint32_t* end, uint32_t* status, uint32_t* link,
                                       uint32_t* length, uint32_t* crc, uint64_t* ntab, uint64_t* counters);

/* ---- report text written block-gzipped (csrc/kr_deflate.h, csrc/kr_dev_deflate.inc; docs/design/15_bgzf_out.md) ----
 * The opposite direction: bytes deflated into BGZF members of at most 65,280 input bytes each (where bgzip cuts), one DEFLATE block
 * a member -- greedy matches from a hash table, fixed Huffman codes, or one stored block when that is not smaller.  One encoder
 * (csrc/kr_deflate.h) runs serially on the host and as one wave per member on the device, and both give THE SAME BYTES for the same
 * input.  Members concatenate: the files of several calls, written one behind the other and ended with kr_bgzf_eof's member, are
 * one BGZF file that zcat, bgzip -d, tabix and kr_batch_submit_bgzf read.
 * No device:
 *   kr_bgzf_deflate_bound   the most bytes kr_bgzf_deflate_host or the device produce for n bytes: n + 31 a member
 *   kr_bgzf_deflate_host    text[0 .. n) as members into out[0 .. cap); n == 0 gives no member.  The members are spread over the host
 *                           thread pool; the bytes do not depend on the thread count.  KR_ERR_CAPACITY when they need more than cap
 *   kr_bgzf_eof             the standard 28-byte empty member that ends a BGZF file
 *   kr_debug_bgzf_deflate_stats   (tests) what the host form did with text[0 .. n): stats[6] = members, stored members, literals,
 *                           matches, longest match, farthest distance (the last four over the coded members)
 * Device:
 *   kr_stream_bgzf_out_enable   once per stream, after kr_stream_text_enable or kr_stream_seek_enable made text buffers (before them,
 *                           or twice: KR_ERR_STATE): device buffers for the members of max_text_bytes of text
 *   kr_batch_collect_text_bgzf  kr_batch_collect_text with the text deflated on the device: the same statuses for the same reasons
 *                           (and KR_ERR_STATE before kr_stream_bgzf_out_enable).  *comp points into the stream's page-locked
 *                           buffer and stays valid until the next submit on this stream; *len: its bytes, *text_len: the bytes
 *                           it inflates to.  No end member is written.  The text stays on the device as it is:
 *                           kr_batch_collect_text on the same batch still returns the plain bytes.  Serves `dist` and KR_SEEK text
 *   kr_debug_bgzf_deflate   (tests) any host bytes through the kernels: out[0 .. cap) receives the members (KR_ERR_CAPACITY: more
 *                           than cap).  Not while a batch is in flight on the stream's first lane (it is waited for)
 *   kr_debug_bgzf_deflate_ms    (measurements) device time (ms) of the deflate, scan and copy kernels of the stream's last deflate;
 *                           -1 before the first
 * Levels.  Level 1 is the encoder above and the default of every call without a level.  Level 2 codes the SAME tokens in a
 * second pass under dynamic Huffman codes built from the member's own counts (BTYPE 10), and keeps level 1's fixed-code or stored
 * block -- the same bytes -- for a member that those make smaller: a level-2 member is never larger than the level-1 member.
 *   kr_bgzf_deflate_host_level     kr_bgzf_deflate_host at a level; KR_ERR_ARG for a level other than 1 or 2
 *   kr_stream_bgzf_out_level       the level of the stream's later kr_batch_collect_text_bgzf and kr_debug_bgzf_deflate calls; after
 *                           kr_stream_bgzf_out_enable (before it: KR_ERR_STATE); KR_ERR_ARG for a level other than 1 or 2, the
 *                           level in force stays.  Level 2 takes a token buffer of 4 bytes per byte of max_text_bytes, made by
 *                           the first call that asks for it.  The level may change between batches
 *   kr_debug_bgzf_deflate_stats_level  (tests) kr_debug_bgzf_deflate_stats at a level: stats[10] = the six figures, then members
 *                           coded with fixed codes, members coded with dynamic codes, members for which one of the three codes
 *                           had to be limited (15 / 15 / 7 bits), dynamic header bits in total
 *   kr_debug_huffman_lengths       (tests) the level-2 code-length builder on the host: lens[0 .. nsym) for the counts
 *                           freq[0 .. nsym) with no code longer than maxbits, *limited = 1 when the limit was needed.  1 <= nsym
 *                           <= 286, 1 <= maxbits <= 15, counts below 2^22, at most 2^maxbits of them non-zero (else KR_ERR_ARG)
 *   kr_debug_huffman_lengths_device  (tests) the same through a kernel of one wave on the stream's device
 * Member length.  A member takes 65,280 input bytes unless the caller says otherwise: any length from 256 to 65,280 is BGZF.  One
 * wave codes one member, so shorter members are more and shorter waves, at a small price in ratio (docs/design/15 section 15.7).
 *   kr_bgzf_deflate_bound_member   kr_bgzf_deflate_bound for members of member_bytes input bytes; 0 for a length outside
 *                           256 .. 65,280
 *   kr_bgzf_deflate_host_member    kr_bgzf_deflate_host_level with members of member_bytes input bytes (the last one shorter);
 *                           65,280 gives kr_bgzf_deflate_host_level's bytes.  KR_ERR_ARG for a length outside 256 .. 65,280
 *   kr_stream_bgzf_member          the member length of the stream's later device deflates (kr_batch_collect_text_bgzf,
 *                           kr_debug_bgzf_deflate, kr_place_stream under kr_stream_place_bgzf) and of the host encoder where
 *                           kr_place_stream uses it.  KR_ERR_ARG outside 256 .. 65,280, the length in force stays.  After
 *                           kr_stream_bgzf_out_enable the buffers are reserved again for the members of max_text_bytes before
 *                           any kernel is queued (a batch in flight is waited for)
 *   kr_debug_bgzf_deflate_at       (tests) kr_debug_bgzf_deflate for a text that starts at any byte: bytes[0 .. n) go to the
 *                           device, [skip, n) is deflated from the device address of byte `skip`
 * `place`.  kr_stream_place_bgzf(stream, level): 0 off (the default), 1 or 2 the encoder's level, anything else KR_ERR_ARG.  It
 * needs neither kr_stream_text_enable nor kr_stream_bgzf_out_enable: the buffers grow with the text.  While it is on,
 * kr_place_stream and kr_place_stream_parsed return BGZF members in *text / *len (no end member) that inflate to exactly the
 * bytes the same call returns with it off; tabular == 2 and an empty text give *len == 0; has_previous, the placement records
 * and every status are unchanged.  A range of reads whose rows were written on the device is deflated there, behind the text
 * kernels, and only the members come back; a range the host formats goes through kr_bgzf_deflate_host_member at the same level
 * and member length.  With one range a call the result is byte for byte kr_bgzf_deflate_host_member of the plain call's text;
 * with several it is the ranges' encodings one behind the other.
 *   kr_place_bgzf_counters         ranges of this process deflated on the device / by the host encoder (either may be null) */
KR_API uint64_t kr_bgzf_deflate_bound(uint64_t n);
KR_API int kr_bgzf_deflate_host(const uint8_t* text, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* len);
KR_API void kr_bgzf_eof(uint8_t* out28);
KR_API int kr_debug_bgzf_deflate_stats(const uint8_t* text, uint64_t n, uint64_t* stats);
KR_API int kr_stream_bgzf_out_enable(kr_stream*);
KR_API int kr_batch_collect_text_bgzf(kr_stream*, const uint8_t** comp, uint64_t* len, uint64_t* text_len);
KR_API int kr_debug_bgzf_deflate(kr_stream*, const uint8_t* bytes, uint64_t n, uint8_t* out, uint64_t cap, uint64_t* len);
KR_API int kr_debug_bgzf_deflate_ms(kr_stream*, float* ms);
KR_API int kr_bgzf_deflate_host_level(const uint8_t* text, uint64_t n, uint32_t level, uint8_t* out, uint64_t cap, uint64_t* len);
KR_API int kr_stream_bgzf_out_level(kr_stream*, uint32_t level);
KR_API int kr_debug_bgzf_deflate_stats_level(const uint8_t* text, uint64_t n, uint32_t level, uint64_t* stats);
KR_API int kr_debug_huffman_lengths(const uint32_t* freq, uint32_t nsym, uint32_t maxbits, uint8_t* lens, uint32_t* limited);
KR_API int kr_debug_huffman_lengths_device(kr_stream*, const uint32_t* freq, uint32_t nsym, uint32_t maxbits, uint8_t* lens, uint32_t* limited);
KR_API uint64_t kr_bgzf_deflate_bound_member(uint64_t n, uint32_t member_bytes);
KR_API int kr_bgzf_deflate_host_member(const uint8_t* text, uint64_t n, uint32_t level, uint32_t member_bytes, uint8_t* out, uint64_t cap, uint64_t* len);
KR_API int kr_stream_bgzf_member(kr_stream*, uint32_t member_bytes);
KR_API int kr_debug_bgzf_deflate_at(kr_stream*, const uint8_t* bytes, uint64_t n, uint64_t skip, uint8_t* out, uint64_t cap, uint64_t* len);
KR_API int kr_stream_place_bgzf(kr_stream*, uint32_t level);
KR_API void kr_place_bgzf_counters(uint64_t* device_ranges, uint64_t* host_ranges);

/* ---- `seek` on kernels of its own (csrc/kr_dev_seek.inc; docs/design/13_seek.md; INTEGRATION.md "A seek batch") ----
 * SBatch::seek_sequences (src/seek.cpp:22-126) on a SKETCH index (kr_host_sketch_load): per k-mer and strand the minimum Hamming
 * distance over one bucket, a histogram of hdist_th + 1 bins per strand, one minimisation per strand, the smaller d -- or NaN when
 * neither strand matched.  A batch flagged KR_SEEK runs these kernels instead of the dist chain: no item list, no record slots, no
 * accumulate scratch; a sequence of any length is split into units of kr_debug_seek_layout's [0] k-mer positions, one wave each,
 * whose counts are added with integer atomics (exact, deterministic).  It runs as one lane, ordered by the index's kernel chain.
 *   kr_stream_seek_enable   once per stream, on a sketch index (else KR_ERR_ARG): the per-read counters and values; with
 *                           max_text_bytes / max_id_bytes (both, or both 0: values only) the id and text buffers, unless
 *                           kr_stream_text_enable made them already (then they must be at least as large: KR_ERR_STATE)
 *   kr_batch_submit(flags | KR_SEEK)        with KR_BASES_HOST, KR_BASES_PINNED or KR_BASES_DEVICE; then kr_batch_collect_seek
 *   kr_batch_submit_text(flags | KR_SEEK)   the same with ids; kr_batch_collect_text returns the report: SEQ_ID '\t' DIST '\n' with
 *                           DIST as "%.5f", or SEQ_ID "\tNaN\n" (byte for byte kr_format_seek's); more text than max_text_bytes:
 *                           KR_ERR_CAPACITY.  kr_batch_collect_seek serves such a batch too
 *   kr_batch_submit_fastq / _fasta(KR_SEEK)   the accepted prefix as a seek batch (text when the stream has text buffers); alone,
 *                           the record finder stops at the first long record as ever (KR_FASTQ_LONG); with KR_SEEK | KR_TILE_DEVICE
 *                           long records are accepted, NO tile layout is built and the seek units do the splitting
 * KR_SEEK is refused (KR_ERR_ARG) with KR_TAP_ACCS, KR_TAP_HITS, KR_ROWS_ONLY, KR_ROWS_INDEXED, KR_TILE_ROWS, and with KR_TILE_DEVICE
 * on kr_batch_submit / kr_batch_submit_text; KR_ERR_STATE when seek was not enabled.  kr_batch_wait serves a seek batch;
 * kr_batch_collect, kr_batch_collect_device and kr_batch_timing give KR_ERR_STATE after one, kr_batch_collect_seek after a batch
 * that was not one, kr_batch_collect_text after a seek batch without ids. */
#define KR_SEEK 256u  /* the batch is a `seek` batch: seek kernels instead of the dist chain (sketch indexes only) */

typedef struct kr_seek_view {
  uint32_t nreads, np;        /* np = hdist_th + 1 */
  const double*   d;          /* [nreads]  reported DIST, NaN: no k-mer of either strand matched */
  const double*   d_strand;   /* [2*nreads] d of the forward / reverse-complement summary (where d is not NaN) */
  const uint32_t* hist;       /* [nreads*2*np] matched k-mers by minimum Hamming distance: read, strand, bin */
  const uint32_t* onmers;     /* [nreads]  valid k-mers */
} kr_seek_view;               /* page-locked, valid until the stream's next submit */

KR_API int kr_stream_seek_enable(kr_stream*, uint64_t max_text_bytes, uint64_t max_id_bytes); /* 0, 0: values only, no text */
KR_API int kr_batch_collect_seek(kr_stream*, kr_seek_view* out);
KR_API int kr_debug_seek_layout(uint32_t* out4);   /* [0] = T (positions per unit), [1] positions per segment, [2] waves per workgroup of the hist kernel, [3] reads per prefix block; no device needed */
KR_API int kr_debug_seek_ms(kr_stream*, float* ms3); /* hist (with the unit count), solve, text of the last seek batch (HIP events) */

/* ---- the reads of a seek batch split by their DIST, on the device (csrc/kr_dev_extract.inc; docs/design/13_seek.md 13.6;
 *      INTEGRATION.md "Reads split by a seek batch") ----
 * A seek batch that a record finder queued (kr_batch_submit_fastq / _fasta / _bgzf with KR_SEEK) has its chunk in device memory, and
 * its accepted records tile the bytes [0, consumed) without a gap.  On a stream with extract enabled those bytes are partitioned
 * behind the solve kernel: a read is MATCHED when its DIST is not NaN and, with a threshold, DIST <= max_dist (compared in double on
 * the value the report text is formatted from).  Every record moves as the exact bytes it has in the chunk -- header comments,
 * qualities, line wrapping, CRLF --, the matched records to the front, the unmatched ones behind them, both in input order; the
 * host only copies and writes.  Nothing else of the batch changes: kr_batch_collect_text / kr_batch_collect_seek give what they give
 * on a stream without extract, and a seek batch from host arrays (kr_batch_submit / _text with KR_SEEK) runs as before and has
 * nothing to extract.
 *   kr_stream_extract_enable   once per stream, after kr_stream_seek_enable and kr_stream_fastq_enable (else, or twice: KR_ERR_STATE);
 *                           max_dist NaN: every read with a DIST is matched; negative or infinite: KR_ERR_ARG.  Allocates the record
 *                           starts, the prefix arrays, one output buffer of the chunk's size and its page-locked mirror
 *   kr_stream_extract_max   another threshold for the batches submitted from now on (KR_ERR_ARG leaves the rule in force as it is)
 *   kr_batch_collect_extract       waits for the batch; copies back the parts named in `which` (KR_EXTRACT_MATCHED | _UNMATCHED;
 *                           0 or an unknown bit: KR_ERR_ARG); a part not asked for has a NULL pointer and length 0, the four counts
 *                           are always filled
 *   kr_batch_collect_extract_bgzf  the same with each non-empty part deflated into BGZF members by the stream's deflate kernels, at
 *                           `level` (1 or 2, else KR_ERR_ARG) and the stream's member length (kr_stream_bgzf_member): byte for byte
 *                           kr_bgzf_deflate_host_member(part, n, level, member_bytes, ...).  An empty part has length 0: no member.
 *                           kr_stream_bgzf_out_enable is not needed; the deflate buffers grow with the parts
 * KR_ERR_STATE from the collect calls: extract not enabled; the last submit was not a raw-bytes seek submit; it accepted no record;
 * the batch was a dist batch.  The pointers are page-locked and stay valid until the stream's next submit (the members' also
 * until a later kr_batch_collect_extract_bgzf call on the same batch overwrites them).
 *
 * PAIRED READS (docs/design/13_seek.md 13.7): the mates of a pair are split together, so that record i of the matched part of file 1
 * is the mate of record i of the matched part of file 2, and the same for the unmatched parts.
 *   kr_stream_extract_defer  between batches, after kr_stream_extract_enable (else KR_ERR_STATE).  on != 0: a raw-bytes seek submit
 *                           queues no extract kernels; the collect calls answer KR_ERR_STATE (naming kr_batch_extract_pair) until
 *                           the pair call.  0: every batch is split by its own reads again (the default)
 *   kr_batch_extract_pair   a and b hold the mates: record r of a's batch and record r of b's; a == b: one interleaved batch, the
 *                           mate of record r is record r ^ 1.  A pair is matched under KR_PAIR_ANY when either mate is matched by
 *                           the rule above, under KR_PAIR_BOTH when both are.  One kernel writes a pair value per record (ANY: the
 *                           smaller distance that is not NaN; BOTH: NaN when either is, else the larger), and the extract kernels
 *                           run on it for each stream; all of it is queued on a's lane, between two events that order it behind
 *                           b's batch and in front of b's next wait.  Afterwards the collect calls work on each stream as ever
 *                           (nmatched: the matched PAIRS).  Calling it again on the same batches, with the other rule for
 *                           instance, overwrites the parts.  kr_batch_collect_text / _seek of both batches are untouched, and
 *                           kr_debug_extract_ms of either stream times all kernels of the call.
 *                           KR_ERR_ARG: a NULL stream, an unknown rule.  KR_ERR_STATE: streams of different kr_index objects; a
 *                           stream without extract or without defer; the last submit of one was not a raw-bytes seek batch, or
 *                           it failed, or accepted no record; different record counts (the message names both); an odd count
 *                           with a == b; different thresholds (they must be bitwise equal, or both NaN). */
#define KR_EXTRACT_MATCHED   1u
#define KR_EXTRACT_UNMATCHED 2u
#define KR_PAIR_ANY  1u
#define KR_PAIR_BOTH 2u
typedef struct kr_extract_view {
  uint32_t nreads, nmatched;
  uint64_t matched_bytes, unmatched_bytes;   /* record bytes of each part (plain) */
  const uint8_t *matched, *unmatched;        /* page-locked, valid until the stream's next submit; NULL when not asked for */
  uint64_t matched_len, unmatched_len;       /* bytes at the pointers: == *_bytes plain, the members' bytes for _bgzf */
} kr_extract_view;
KR_API int kr_stream_extract_enable(kr_stream*, double max_dist);   /* NaN: every read with a finite DIST is matched */
KR_API int kr_stream_extract_max(kr_stream*, double max_dist);      /* between batches */
KR_API int kr_batch_collect_extract(kr_stream*, uint32_t which, kr_extract_view* out);
KR_API int kr_batch_collect_extract_bgzf(kr_stream*, uint32_t which, uint32_t level, kr_extract_view* out);
KR_API int kr_debug_extract_ms(kr_stream*, float* ms);              /* the extract kernels of the last batch, HIP events */
KR_API int kr_stream_extract_defer(kr_stream*, uint32_t on);        /* between batches */
KR_API int kr_batch_extract_pair(kr_stream* a, kr_stream* b, uint32_t rule);
/* tests: the tiled form of the batch last submitted on the stream as it lies on the device, laid out by the host (a host batch)
 * or by kernels (KR_TILE_DEVICE): reads of the tiled batch and long sequences; voff [nv + 1] where every read of the tiled batch
 * starts in its bases, vtile [nv] 1 = a tile of a long sequence, rfirst [nreads] the caller's read's first read of the tiled batch,
 * longs [2 * nlong] (first tile, tiles) of every long sequence, bases [voff[nv]].  *nv == 0: the batch is not tiled (nothing else
 * is written).  Any array pointer may be NULL. */
KR_API int kr_debug_tile_layout(kr_stream*, uint32_t* nv, uint32_t* nlong, uint64_t* voff, uint8_t* vtile, uint32_t* rfirst,
                                uint32_t* longs, uint8_t* bases);
/* tests (no device needed): a sequence of `len` bases as the tilers see it -- k-mer positions, tiles of 128 positions, and the
 * bases it takes in a tiled batch (every tile but the first repeats k - 1 bases) */
KR_API int kr_debug_tile_shape(uint64_t len, uint32_t k, uint64_t* nkm, uint64_t* nt, uint64_t* bytes);

/* ------------------------------------------------------------------------- */
/* `krepp place`: IBatch::place_sequences / report_placement (src/query.cpp:198-333), */
/* TargetIndex::ensure_backbone (src/krepp.cpp:48-64), Tree::map_to_qtree /           */
/* compute_eff_nchildren (src/phytree.cpp:421-473); lineage trees: read_lineages         */
/* (src/krepp.cpp:37-46), Tree::parse_lineages (src/phytree.cpp:320-369).               */
/* ------------------------------------------------------------------------- */
typedef struct kr_place_tree kr_place_tree;
/* nwk_text == NULL: place on the index's own backbone; otherwise map the index leaves onto the
 * given rooted Newick tree.  kr_place_tree_kinds gives the node_kind array to upload the index
 * with (leaves absent from the placement tree become null nodes, as after map_to_qtree). */
KR_API int kr_place_tree_create(const kr_host_index*, const char* nwk_text, kr_place_tree** out);
/* -l/--lineage-file: the placement tree is the taxonomy of a Greengenes/GTDB style lineage file
 * (`ID <tab> r__Taxon; r__Taxon; ...` per line); its leaves are the reference IDs. */
KR_API int kr_place_tree_create_lineage(const kr_host_index*, const char* lineage_text, kr_place_tree** out);
KR_API uint32_t kr_place_tree_nnodes(const kr_place_tree*);
KR_API void kr_place_tree_free(kr_place_tree*);
KR_API const uint8_t* kr_place_tree_kinds(const kr_place_tree*);

typedef struct kr_placement {
  uint32_t read;
  uint32_t edge;  /* Node::get_en = se - 1 in the placement tree */
  double lwr, d_llh, v_llh, pendant, distal;
} kr_placement;

/* Back end for one collected batch.  `rv` must come from kr_batch_collect of a stream created with
 * multi = 1, no_filter = 1, dist_max unset, submitted with KR_TAP_ACCS (it needs the histograms);
 * `p` carries the place options (tau, chisq, multi, no_filter; filter defaults to on for place,
 * src/krepp.cpp:593-630).  The tree aggregation runs on the host; every likelihood (Brent on the
 * fractional histograms of internal nodes, the chi-square evaluations) runs on the GPU through
 * kr_llh_batch.  `has_previous` carries the jplace comma state across batches (in/out). */
KR_API int kr_place_batch(const kr_host_index*, const kr_index*, const kr_place_tree*, const kr_result_view* rv,
                          const uint64_t* offsets, const char* const* names, const kr_params* p, int tabular,
                          int* has_previous, char** text, uint64_t* len, kr_placement** placements, uint64_t* nplacements);
/* The same for the batch last submitted on `s` (KR_TAP_ACCS; no collect needed): the whole back end of
 * report_placement up to the candidate list -- ancestor accumulation (Minfo::add, src/query.hpp:139-152;
 * src/query.cpp:248-265), candidate listing (:268-272), Brent on the internal candidates (:273-275) and the
 * chi-square of every candidate (:276) -- runs on the device, on the records where they lie; the host receives
 * the candidates and does the last phase (filter, LWR, Jukes-Cantor, text).  Output identical to kr_place_batch.
 * Reads of any weight stay on the device (see kr_place_counters). */
KR_API int kr_place_stream(const kr_host_index*, const kr_index*, const kr_place_tree*, kr_stream* s, uint32_t nreads,
                           const uint64_t* offsets, const char* const* names, const kr_params* p, int tabular,
                           int* has_previous, char** text, uint64_t* len, kr_placement** placements, uint64_t* nplacements);
/* The same for the batch that kr_batch_submit_fastq or kr_batch_submit_fasta queued last on `s`: reads given as raw file bytes are
 * placed without a host array of offsets, names or lengths.  The submit must have carried KR_TAP_ACCS (KR_TILE_DEVICE may be added:
 * long records are tiled on the device, the caller's reads are placed) and accepted at least one record.  nreads, the offsets and
 * the names are the stream's own: the reads' lengths are taken from the record finder's offsets and their ids are gathered from the
 * chunk, both by kernels on the stream, behind the batch; the output is byte for byte, and placement record for placement record,
 * what kr_place_stream gives for the same reads under the same names.
 *   raw    the pointer given to that submit; it stays valid through this call and is read only where the HOST formats: the whole
 *          batch on the host back end, a range whose device text is not used (KR_PLACE_HOST_TEXT, a text flag, `placements`
 *          wanted with rows).  Only those paths copy the offsets or the names' (position, length) pairs back; with device text
 *          (tabular 0 or 1, no placements) the call reads back one number more than kr_place_stream: the ids' total, which sizes
 *          the id and text buffers exactly.
 * The chunk, the names' positions and lengths and the offsets stay in HBM, untouched, from the submit to the stream's next submit
 * (the tiling kernels of KR_TILE_DEVICE and a batch run again by kr_batch_wait write none of them).
 * KR_ERR_STATE: the last submit on `s` was not a raw-bytes submit, accepted no record (nothing was queued), or lacked KR_TAP_ACCS;
 * KR_ERR_ARG: a null argument (`placements` / `nplacements` may be null); KR_ERR_CAPACITY: as kr_place_stream, or 4 GB of ids. */
KR_API int kr_place_stream_parsed(const kr_host_index*, const kr_index*, const kr_place_tree*, kr_stream* s, const uint8_t* raw,
                                  const kr_params* p, int tabular, int* has_previous, char** text, uint64_t* len,
                                  kr_placement** placements, uint64_t* nplacements);
/* tests: the reads' ids as the device laid them out for the stream's last kr_place_stream_parsed call that wrote text on the device:
 * id_off [nreads + 1] (id_off[0] = 0), ids [id_off[nreads]] back to back.  KR_ERR_STATE after any other place call. */
KR_API int kr_debug_place_ids(kr_stream*, char* ids, uint32_t* id_off);
/* How many kr_place_stream batches of this process ran their back end on the device, and how many were sent whole to the
 * host back end (kr_place_batch: a placement tree that is not numbered in post-order, KR_PLACE_HOST set, or a batch that ran
 * out of candidate slots); heavy_reads: reads with more leaves / distinct ancestors than kr_place_kernel's LDS arrays hold
 * (256 / 1024), which its second launch does with the arrays in global scratch (counted in list chunks of 8: an upper
 * bound, 0 when there was none).  Any pointer may be NULL. */
KR_API void kr_place_counters(uint64_t* device_batches, uint64_t* host_batches, uint64_t* heavy_reads);
/* Ranges of reads whose `place` rows were written on the device / that the host formatted although device text was asked for. */
KR_API void kr_place_text_counters(uint64_t* device_ranges, uint64_t* fallback_ranges);
/* Which recovery paths of the device back end ran in this process: the first `n` (at most KR_PLACE_PATHS) of
 *   [0] ranges run again because the candidate slots ran out (once per rerun)   [1] ... because the kept-candidate slots ran out
 *   [2] ranges finished with the internal candidates' list incomplete (kr_place_llh_kernel minimised by itself)
 *   [3] ranges given up: still out of slots after two reruns, or asking for more than a slot index can name (the batch goes to
 *       the host back end)
 *   [4..8] ranges whose device text was not taken, by flag: 1 a number out of range, 2 more text than the buffer holds, 4 (not
 *       raised any more), 8 a rounding tie too close, 16 nothing formatted / a node number out of range; a range counts once
 *       under every flag it raised
 *   [9] ranges finished
 *   of the range finished last, its last attempt: [10] candidate slots asked for  [11] kept-candidate slots handed out  [12]
 *   entries of the internal candidates' list handed out  [13] bytes of its text (0 without device text)  [14] [15] [16] the
 *   candidate slots, kept slots and text bytes it ran with  [17] its flag word  [18] its text flags  [19] attempts (1: no rerun).
 * [0..9] only grow.  For tests (KR_DEBUG_PLACE_CAPS lowers the capacities). */
#define KR_PLACE_PATHS 20
KR_API void kr_place_path_counters(uint64_t* out, uint32_t n);
/* Tests (no device needed): the constants the per-read kernel of `place` is compiled with: out8 = {leaves of a read the LDS arrays hold
 * (kPlLeaves), distinct ancestors (kPlNodes), leaves an ancestor's lane handles at a time (kPlBlock), (leaf, ancestor) weights a wave's
 * global scratch holds (kPlChain), candidate slots a wave takes at a time (kPlChunk), the factor of the chained threshold (weights go
 * through the scratch where their number exceeds factor * leaves), most leaves of a read whose ancestor lanes walk their own run of
 * the leaf list, the multiple of kPlChain a wave of the first launch has for a read it does in global scratch}. */
KR_API int kr_debug_place_layout(uint32_t* out8);
/* Tests: path witnesses of the per-read kernel of `place`, counted only in calls made under KR_DEBUG_PLACE_PATHS=1 (read per call) and
 * summed over the ranges finished in this process (the last attempt of each): the first min(n, 12) into `out`, in this order -- reads
 * whose (leaf, ancestor) weights went through global scratch, whose weights were walked on a shallow tree, walked because they exceed
 * the scratch, whose histograms were re-read from the records, whose ancestor lanes walked the whole leaf list, with a record dropped
 * for a later one on its node, single placements, reads stopped by the tau gate of their closest leaf, reads finished with their arrays
 * in the first launch's LDS, in global scratch by the first launch, by the second launch, ancestor lanes that took more than one block
 * of leaves.  All but the single placements and the tau gate count reads of two leaves or more that got their candidate slots. */
KR_API void kr_debug_place_paths(uint64_t* out, uint32_t n);
/* `tabular`: 0 jplace, 1 --tabular, 2 --summarize (no per-read text; feed the placements to
 * kr_place_summary_add).  place --summarize (src/krepp.cpp:466-471,493-497): `wcount` has
 * kr_place_tree_nnodes + 1 doubles, zeroed by the caller before the first batch and indexed by edge + 1. */
KR_API int kr_place_summary_add(const kr_place_tree*, const kr_placement* placements, uint64_t n, double* wcount,
                                double* twcount);
KR_API int kr_place_summary_text(const kr_place_tree*, const double* wcount, double twcount, char** text, uint64_t* len);
/* which = 0: text before the batches (jplace opening / tabular or summary header), 1: after (jplace metadata + tree) */
KR_API int kr_place_frame(const kr_place_tree*, int which, int tabular, const char* invocation, uint64_t total_qseq,
                          char** text, uint64_t* len);

/* Index construction (`krepp index`, src/krepp.cpp:131-303); needed to make any index at all.  On the CPU by default, as in
 * the reference.  `gpu_minimizers` is a bit set that moves stages to the GPU `device`, with identical files:
 *   KR_BUILD_GPU_MINIMIZERS  the leaf stage (window minimizers of every genome; kr_minimizers_device)
 *   KR_BUILD_GPU_KEYS        also the key stage: all genomes' keys stay in a device pool and are sorted and grouped there
 *                            (kr_key_groups_device); implies the leaf stage.  The colours of the groups stay on the host.
 *   KR_BUILD_GPU_COLOURS     also the colour classes: the distinct leaf sets among the groups are found on the device while the
 *                            groups are still there (kr_colour_classes_device), and the host folds each set into a colour once
 *                            instead of once per key; implies the key and the leaf stage. */
#define KR_BUILD_GPU_MINIMIZERS 1u
#define KR_BUILD_GPU_KEYS 2u
#define KR_BUILD_GPU_COLOURS 4u          /* implies KR_BUILD_GPU_KEYS and KR_BUILD_GPU_MINIMIZERS */
typedef struct kr_build_params {
  uint32_t k, w, h, m, r, frac; /* defaults 29, 35, 13, 4, 1, 1 (src/krepp.hpp:47-58) */
  uint32_t num_threads;
  uint32_t seed;
  const uint8_t* ppos;          /* optional explicit LSH positions [h] (descending)    */
  uint32_t gpu_minimizers;      /* bit set KR_BUILD_GPU_*: 1 leaf stage, 2 key stage too, 4 colour classes too, on the GPU `device`; */
  int32_t device;               /*    identical output, checked by tests/test_minimizers.py, test_gpu_build_keys.py, test_gpu_build_colours.py */
  uint32_t sdust_t, sdust_w;    /* --sdust-t / --sdust-w (src/krepp.cpp:530-531,576-577): both > 0 keeps the sdust intervals  */
                                /* of every contig out of the minimizer windows (src/rqseq.cpp:71-107); either 0: off    */
} kr_build_params;
KR_API int kr_build_index(const char* input_tsv, const char* nwk_path /*may be NULL*/, const char* out_dir,
                          const kr_build_params*);
/* `krepp sketch` (SketchSingle::create_sketch / save_sketch, src/krepp.cpp:110-129): the minimizers of one
 * FASTA/FASTQ file in the reference's sketch format (defaults there: k 26, w k+6, h k-16, m 4, r 1, frac). */
KR_API int kr_build_sketch(const char* input_path, const char* out_path, const kr_build_params*);

/* The leaf stage of the build on its own: RSeq::extract_mers (src/rqseq.cpp:51-144) + the
 * sort/unique of DynHT::fill_table (src/table.cpp:247-260) for ONE genome held in memory
 * (contigs concatenated, offsets[ncontigs+1]).  keys = (row << 32) | enc32, sorted, unique;
 * n1/n2 = sums over contigs of the HyperLogLog(12) estimates of distinct k-mers / distinct
 * window minimizers (rho = n2 / n1, src/rqseq.hpp:79).  `ppos` must be given.
 * _cpu is the builder's own code path; _device computes the window minima on the GPU
 * (wave ballots for the 2-bit strings, LDS window minimum) and must return identical results. */
typedef struct kr_minimizer_result {
  uint64_t* keys;
  uint64_t nkeys;
  double n1, n2;
} kr_minimizer_result;
KR_API int kr_minimizers_cpu(const kr_build_params*, const uint8_t* bases, const uint64_t* offsets, uint32_t ncontigs,
                             kr_minimizer_result* out);
KR_API int kr_minimizers_device(int device, const kr_build_params*, const uint8_t* bases, const uint64_t* offsets,
                                uint32_t ncontigs, kr_minimizer_result* out);
KR_API void kr_minimizers_free(kr_minimizer_result*);

/* The key stage of the build on its own: n (key, leaf rank) pairs in any order, whole pairs possibly repeated, come back sorted by
 * (key, rank) without duplicates and cut into groups of equal key, with the cumulative row counts of the inc-* file.
 * KR_ERR_FORMAT ("row out of range") if a key's row is >= nrows; KR_ERR_ARG if a rank is >= nleaves or nleaves > 65536.
 * _cpu is the builder's own host path (one comparison sort, one walk over the runs); _device is a least-significant-digit
 * radix sort (8-bit digits, the rank's first, only digits that can differ) and a flag / scan / scatter grouping on the GPU and
 * must return identical arrays. */
typedef struct kr_key_groups {
  uint64_t* keys;    /* [nkeys]  distinct keys, ascending: (row << 32) | enc32                              */
  uint64_t* goff;    /* [nkeys + 1] group i owns ranks[goff[i] .. goff[i+1])                                  */
  uint32_t* ranks;   /* [npairs] leaf ranks of a group ascending, each once                                   */
  uint64_t* inc;     /* [nrows]  number of distinct keys with row <= r (what inc-* holds)                     */
  uint64_t nkeys, npairs;
  uint32_t nrows;
} kr_key_groups;
KR_API int kr_key_groups_cpu(const uint64_t* keys, const uint32_t* ranks, uint64_t n, uint32_t nrows, uint32_t nleaves, kr_key_groups* out);
KR_API int kr_key_groups_device(int device, const uint64_t* keys, const uint32_t* ranks, uint64_t n, uint32_t nrows, uint32_t nleaves, kr_key_groups* out);
KR_API void kr_key_groups_free(kr_key_groups*);
/* Tests: the calling process's last kr_key_groups_device or GPU key build (KR_BUILD_GPU_KEYS): {pairs in, pairs out, keys out,
 * radix passes run, pool growths, path taken (1 device, 2 fell back to the host for memory, 3 fell back for more than 65,536
 * leaves), pairs per tile of the sort, 0}. */
KR_API void kr_debug_build_keys(uint64_t out[8]);

/* The colour classes of key groups (goff / ranks as kr_key_groups lays them out; goff[0] = 0, goff ascending): a class is one
 * distinct rank sequence among the groups of two or more ranks.  Both functions hold these invariants:
 *   every group of a class has exactly the ranks of group rep[class];
 *   rep[c] is the smallest group index in class c and rep ascends, so that classes are numbered in order of first appearance;
 *   a group of fewer than two ranks has KR_NO_CLASS.
 * _cpu is the canonical form, exactly one class per distinct set (a hash map on the host).  _device sorts 64-bit fingerprints of the
 * sets (a wrapping sum of hashed ranks plus a hashed length, from one scan over all ranks) and compares every group's ranks with
 * those of its predecessor in that order; it gives the canonical form unless two different sets share a fingerprint, in which case
 * a set may be split over several classes, each led by its own smallest group index.  When the device has no room the classes
 * come from _cpu (never an error).  KR_BUILD_COLOUR_HASH_BITS=N (environment, read at each call, default 64) keeps only the low N
 * bits of every fingerprint: a knob for tests of the content compare. */
#define KR_NO_CLASS 0xFFFFFFFFu
typedef struct kr_colour_classes {
  uint32_t* class_of;  /* [nkeys]    class of group i; KR_NO_CLASS for a group of one rank                    */
  uint64_t* rep;       /* [nclasses] a group index per class, strictly ascending: the class's FIRST group      */
  uint64_t nkeys, nclasses;
} kr_colour_classes;
KR_API int kr_colour_classes_cpu(const uint64_t* goff, const uint32_t* ranks, uint64_t nkeys, kr_colour_classes* out);
KR_API int kr_colour_classes_device(int device, const uint64_t* goff, const uint32_t* ranks, uint64_t nkeys, kr_colour_classes* out);
KR_API void kr_colour_classes_free(kr_colour_classes*);
/* Tests: the calling process's last kr_colour_classes_device or index build: {groups, groups of >= 2 ranks, classes, classes whose
 * fingerprint equals their predecessor's in the sorted list (raised by the content compare alone), path (0 not asked, 1 device,
 * 2 host), sort passes, 0, 0}. */
KR_API void kr_debug_build_colours(uint64_t out[8]);

/* The masker on its own: per contig the list that the reference's sdust(0, seq, -1, T, W, &n) (src/sdust.h) returns, element for
 * element: intervals[offsets[c] .. offsets[c+1]) = (start << 32 | finish), finish exclusive.  Its alphabet is sdust's own (bytes
 * 0..3 and ACGTacgt are bases); an interval may cover non-bases and, behind one, reach up to W bases past the contig's end, as
 * the reference's do.  T > 0, W >= 4, contigs below 2^31 bases. */
typedef struct kr_sdust_result {
  uint64_t* intervals;
  uint64_t* offsets; /* [ncontigs + 1] */
  uint32_t ncontigs;
} kr_sdust_result;
KR_API int kr_sdust_cpu(const uint8_t* bases, const uint64_t* offsets, uint32_t ncontigs, uint32_t T, uint32_t W, kr_sdust_result* out);
KR_API void kr_sdust_free(kr_sdust_result*);

/* ------------------------------------------------------------------------- */
/* `krepp inspect` (Index::display_info src/index.cpp:172-186, FlatHT::display_info src/table.cpp:262-270,
 * CRecord::display_info src/record.cpp:257-276): per library the k-mers that carry each colour, the times each colour is named as
 * a child in se_to_pse[1 ..], and how many of the colours 1 .. nsubsets-1 share each of those two figures.
 * _cpu is the canonical form and needs no device.  _device counts on the GPU (kr_index_stats.hip; big arrays from host memory, or
 * from device memory with KR_VIEW_DEVICE) and returns identical arrays; when the device has no room, it finishes through _cpu
 * (never an error).  A colour id >= nsubsets in cmer or in a child of se_to_pse[1 ..] is KR_ERR_FORMAT on both: the message names the
 * library's suffix, the array, the first offending position and the value; `out` holds nothing then.
 * Environment, read at each _device call: KR_STATS_CHUNK_KMERS (cmer entries per chunk), KR_STATS_MAX_MB (cap on the device memory
 * the call may ask for; above it: _cpu), KR_STATS_LDS_CAP (colour ids below it are counted in LDS; 0: global atomics only). */
typedef struct kr_lib_stats {
  uint64_t nkmers;
  uint32_t nsubsets, r, frac;
  uint64_t *mer_value, *mer_freq; /* [n_mer] ascending mer_value; sum(mer_freq) == nsubsets - 1 */
  uint64_t n_mer;
  uint64_t *deg_value, *deg_freq; /* [n_deg] ascending deg_value; sum(deg_freq) == nsubsets - 1 */
  uint64_t n_deg;
  uint64_t* se_count;  /* [nsubsets] k-mers per colour, only with KR_STATS_KEEP_COUNTS, else NULL */
  uint64_t* se_outdeg; /* [nsubsets] likewise */
} kr_lib_stats;
typedef struct kr_index_stats {
  uint32_t nlibs;
  kr_lib_stats* libs;
} kr_index_stats;
#define KR_STATS_KEEP_COUNTS 4u /* beside KR_VIEW_HOST / KR_VIEW_DEVICE in `flags` */
KR_API int kr_index_stats_cpu(const kr_index_view*, uint32_t flags, kr_index_stats* out);
KR_API int kr_index_stats_device(const kr_index_view*, int device, uint32_t flags, kr_index_stats* out);
KR_API void kr_index_stats_free(kr_index_stats*);
/* The metadata text of library `lib` as `inspect` prints it: the content of metadata<suffix>.txt, or the reference's thirteen
 * `name: value` lines (src/index.cpp:128-141) where the file is missing.  "" for a bad argument. */
KR_API const char* kr_host_index_lib_info(const kr_host_index*, uint32_t lib);
/* The text of `krepp inspect`: blocks by ascending residue key, rows by ascending value.  kr_free(*text). */
KR_API int kr_format_inspect(const kr_host_index*, const kr_index_stats*, char** text, uint64_t* len);
/* Tests: the calling process's last kr_index_stats_device: {path (1 device, 2 fell back to the host for memory), cmer chunks,
 * increments served from LDS, increments sent as global atomics, LDS counter capacity in colours, sort passes of the MER_COUNT
 * histogram, sort passes of the OUTDEGREE_COUNT histogram (both of the last library), cmer entries of one workgroup's run}.
 * kr_debug_index_stats_ms: {H2D copies, count kernels, out-degrees and histograms, whole call} in milliseconds (events; the last wall). */
KR_API void kr_debug_index_stats(uint64_t out[8]);
KR_API void kr_debug_index_stats_ms(float out[4]);

KR_API const char* kr_last_error(void);
KR_API const char* kr_version(void);

#ifdef __cplusplus
}
#endif
#endif
