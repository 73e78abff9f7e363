// kr_dev_common.inc -- part of kr_device.hip (one translation unit, included in order): constants, device structs and helpers shared by the kernels.

// ---------------------------------------------------------------------------
// Compile-time shape of the probe kernel
// ---------------------------------------------------------------------------
constexpr int kWave = 64;
constexpr int kSegPos = 128;      // k-mer positions per segment = 4 plane words
constexpr int kPlaneWords = kSegPos / 32;
constexpr int kMaxLibs = 16;
constexpr int kStackCap = 256;    // colour work stack (items of 8 B)
constexpr int kLeanStack = 192;   // ... of the single-segment accumulate instantiation (128 pushes per step + DAG depth)
// its stack region also hosts the key bitmap (4 B per word) and the ordinal prefix (1 B per word)
__host__ __device__ inline uint32_t lean_stack_bytes(uint32_t bm_words) { uint32_t b = 5u * bm_words; b = (b + 15u) & ~15u; return b > kLeanStack * 8u ? b : kLeanStack * 8u; }
constexpr int kLdsSlots = 64;     // level-1 (LDS) accumulator slots per wave: lane t owns slot t in the epilogue
// single-segment accumulate instantiation: resident waves per SIMD its registers are sized for, and the words of its
// event / batch region in LDS (0: as large as the level-1 plane region of the other instantiation)
// (24 waves per CU since the read index is scalar: 80 VGPRs without a spill, 96 with spills before; 6.6 KB of LDS per wave)
#ifndef KR_ACC_LEAN_WPE
#define KR_ACC_LEAN_WPE 6
#endif
#ifndef KR_ACC_PIPE
#define KR_ACC_PIPE 1 // read-ahead over the item tiles of a read in the accumulate kernel (-3 % on the kernel)
#endif
#ifndef KR_ACC_LEAN_EV_WORDS
#define KR_ACC_LEAN_EV_WORDS 1216 // 512 events in LDS (a 150-bp read has 175 on the 1000-genome index), the rest keys and planes
#endif
#ifndef KR_ACC_LEAN2_EV_HALVES
#define KR_ACC_LEAN2_EV_HALVES 4 // event / batch region of the two-segment instantiation, in halves of the one-segment region
#endif
__host__ __device__ inline uint32_t lean_ev_words(uint32_t np, uint32_t segs = 1)
{ // (two segments: twice the events, planes of twice the bits)
  const uint32_t w = KR_ACC_LEAN_EV_WORDS ? (uint32_t)KR_ACC_LEAN_EV_WORDS : (uint32_t)kLdsSlots * np * 5u /* kPlaneWords + 1 */;
  return segs == 1 ? w : (w * (uint32_t)KR_ACC_LEAN2_EV_HALVES / 2u + 3u) & ~3u;
}
// Event region of an accumulate instantiation: its words, and how many of them hold events before a read's events spill to the wave's
// global scratch (the rest: keys, planes, counters).  One function for the kernel and for the host (kr_debug_acc_layout).
#ifndef KR_ACC_FAST_EPILOGUE
#define KR_ACC_FAST_EPILOGUE 1
#endif
constexpr uint32_t kFastKeyWords = 7u; // finalize_events_fast: words per key of a batch (its rank, the position map's four, the counters' two)
struct AccLayout {
  uint32_t ev_words, ev_cap;
};
__host__ __device__ inline AccLayout acc_layout(uint32_t np, uint32_t segs, bool multi)
{
  AccLayout l;
  l.ev_words = multi ? (uint32_t)kLdsSlots * np * 5u /* kPlaneWords + 1 */ : lean_ev_words(np, segs);
  l.ev_cap = 64;
  while (l.ev_cap * 2 <= l.ev_words) l.ev_cap <<= 1;
  if (l.ev_cap == l.ev_words) l.ev_cap >>= 1;
  // a small region keeps room for keys and planes -- but not where finalize_events_fast finishes the reads (th = 4): it drops two
  // thirds of a crowded read's events before it needs the room, and events that need not spill are worth more (round 5: 1,024
  // events of the 1,216 words instead of 512: 17.1 -> 16.1 ms per 8 M reads, 38.1 -> 36.0 on the 10,000-genome index)
  if (!multi && KR_ACC_LEAN_EV_WORDS && l.ev_cap * 4u > l.ev_words * 3u && !(KR_ACC_FAST_EPILOGUE && segs == 1 && np == 5u)) l.ev_cap >>= 1;
#ifdef KR_ACC_EV_CAP // (experiments: a multiple of 64)
  if (!multi && segs == 1) l.ev_cap = KR_ACC_EV_CAP;
#endif
  return l;
}
constexpr int kLdsProbeMax = 8;   // bounded probe sequence of the level-1 table
constexpr int kMaxPlanes = KR_MAX_HDIST_TH + 1;
constexpr int kHistWords = (kMaxPlanes + 3) / 4; // packed 8-bit histogram counters

// words per slot of a slot format code (0: no slotted copy)
constexpr uint32_t kSlotFilter = 9u; // format 9: FILTER slots (kr_dev_scan_filt.inc): two 128-byte lines of 24-bit codes
__host__ __device__ inline uint32_t slot_words(uint32_t code) { return code == 0 ? 0u : (code == 8 ? 48u : (code == kSlotFilter ? 64u : 1u << code)); }

// ---------------------------------------------------------------------------
// Filter slots (format 9).  The scan pays per 128-byte LINE it requests (scripts/bin_probe.hip, scripts/filt_probe.hip), and a
// bucket of 37 four-byte codes is two lines.  A filter slot holds the bucket as 24-bit codes -- 12 of the 16 non-LSH positions:
// bits 0..11 of each half of the residual code (src/lshf.cpp:64-69) -- 40 to a line, so that a probe reads ONE line unless its
// bucket has more than 40 entries (Poisson(37): 28 %), and then the second line of the same slot:
//   slot of row r = 16 chunks of 16 bytes; chunk c = 5 codes (entries 5c .. 5c+4 of the bucket, 3 bytes each) + 1 byte:
//   bits 0..2 the number of valid codes in the chunk, bit 7 (chunks 0..7) the bucket goes on in the second line, bit 6
//   (chunks 8..15) the bucket has more than 80 entries (the rest is scanned in the packed arrays, on the spot).
// hd12 <= th on the 12 positions is NECESSARY for hd <= th (src/common.hpp:175 counts positions that differ): an entry that
// passes is a CANDIDATE; the accumulate kernel, which gathers the entry's colour anyway, finds the other 4 positions' bits
// beside the colour -- sx[row * 80 + e] = {tagged colour id, rest bits} -- completes hd and drops the false candidates
// (12.6 per read on the 10 GB table, next to 71 true hits).  hdist_filt (src/query.cpp:366-368) moves with it.
// ---------------------------------------------------------------------------
constexpr uint32_t kFiltLineCodes = 40u, kFiltSlotCodes = 80u;
constexpr uint32_t kFiltMaxTh = 6u; // the candidate's hd12 travels in 3 bits (7 = "verified entry of the packed arrays")
__host__ __device__ inline uint32_t filt_code24(uint32_t enc) { return (enc & 0xFFFu) | ((enc >> 4) & 0xFFF000u); }
__host__ __device__ inline uint32_t filt_rest8(uint32_t enc) { return ((enc >> 12) & 0xFu) | ((enc >> 24) & 0xF0u); }

struct DevLib {
  const uint64_t* bkt;  // [nrows]  (start << 24) | len
  const uint32_t* enc;  // [nkmers + pad] residual codes, bucket-contiguous
  const uint32_t* se;   // [nkmers] colour ids
  const uint2* pse;     // [nsubsets] colour DAG: colour = union of .x and .y
  const double* rho;    // [nnodes] subsampling rates, already scaled
  const uint32_t* slots; // [nrows * slot_words(slot_log2w)] slotted copy of the head of every bucket (dense tables), or null
  const uint32_t* occ;   // [ceil(nrows / 32)] one bit per row: the bucket is not empty (sparse tables), or null
  const uint32_t* leaflist; // [nlist] leaf ranks of the "flat" colours that are not runs, colour after colour (ascending per colour)
  const uint2* sx;       // [nrows * 80] filter slots only (format 9): {tagged colour id, rest bits} of slot entry e of row r at r * 80 + e
  uint64_t nkmers, nlist;
  uint32_t nrows, nsubsets, nnodes, numer;
  uint32_t slot_log2w;  // slot format: 5 / 6 / 7 = 32 / 64 / 128 words, 8 = 48 words (192 bytes); slot = {len, start, first (words - 2) residual codes};
                        // 9 = filter slots (above)
};

struct DevIndex {
  uint32_t k, h, m, nlibs, tree_nnodes;
  uint32_t m_shift;      // log2(m) if m is a power of two, else 0xFFFFFFFF
  PextMask pmask, nmask; // bit masks of the LSH / non-LSH positions within the k-bit half-codes
  const uint4* fe_tab;     // [4 * 256] byte tables of the table-driven front end (front_end_tab below), built at upload
  uint64_t ppk[2], npk[2]; // the same positions for the bit-plane front end: 5 bits each, 12 to a word, DESCENDING (the order it consumes them;
                           // scalar shifts take them out: a byte array indexed in a loop would be fetched by vector loads)
  uint32_t nleaves;
  const uint32_t* node_info; // [tree_nnodes+1] kind (0 null, 1 leaf, 2 internal) | leaf_rank << 2
  const uint32_t* leaf_se;   // [nleaves] colour id of the leaf with a given rank (ranks follow se order)
  const int32_t* res_lib; // [m] library serving each residue, or -1
  const DevLib* libs;    // [nlibs] in device memory
  uint64_t res_mask;     // nlibs == 1 && m <= 64: bit r set iff residue r is served
  DevLib lib0;           // copy of libs[0]: single-library indexes never touch `libs`
};

struct LlhConst {
  uint32_t k, h, th, dbg; // dbg (KR_DEBUG_LLH): bit 0 = the device library's pow in place of pown_dd (llh_dpart; tests/test_gpu_llh_numerics.py relies on it)
  double binom_k[32];
  double binom_hnk[kMaxPlanes];
};

struct DevParams {
  uint32_t th, np;       // np = th + 1 planes
  uint32_t multi, no_filter, dmax_set;
  uint32_t dbg; // KR_DEBUG_SKIP (timing experiments / tests only): 1 drop hits, 2 drop expansion, 4 skip scan, 8 no event mode,
                // 16 drop events, 64 no batches, 128 no plane pass, 256 no record output, 512 statistics, 1024 never / 2048
                // eagerly use the global single batch, 4096 planes for single-event keys too, 8192 plane tables for reads of
                // several segments
  double chisq, dist_max;
};

// Slots of BatchOut::counters: the words a batch's kernels share, one set per lane, cleared before the lane's first kernel and
// copied to the host behind its last.  Behind every meaning: how kr_batch_wait combines the lanes' values (kCounterRules in
// kr_host_stream.inc) -- sum, max, or -- or "lane": read per lane, never combined.
enum CounterSlot : uint32_t {
  kCtRecSlots = 0,      // record slots handed out, in chunks (beyond rec_cap: the lane is over capacity) -- lane
  kCtErr = 1,           // error flags (kErr* below) -- or
  kCtL2Reads = 2,       // reads that used the level-2 (global) accumulator: kr_timing.overflow_reads -- sum
  kCtTapHits = 3,       // hits written to the tap (KR_TAP_HITS), beyond hit_cap too -- sum
  kCtRecords = 4,       // records written -- sum
  kCtLlhCursor = 5,     // chunk cursor of kr_llh_kernel over the distinct problems -- lane
  kCtItemSlots = 6,     // item slots handed out by the scan -- lane
  // KR_DEBUG_SKIP=512 statistics of the accumulate kernel ([kr stats])
  kCtStEvents = 9,      // events -- sum
  kCtStKeys = 10,       // keys -- sum
  kCtStBatches = 11,    // key batches -- sum
  kCtStBig = 12,        // reads beyond the LDS event region -- sum
  kCtStLevelTiles = 13, // level passes x event tiles -- sum
  kCtStMaxKeys = 14,    // most keys of a read -- max
  kCtStMaxEvents = 15,  // most events of a read -- max
  kCtCycLevel = 16,     // wave cycles / 64 in the level passes -- sum
  kCtCycFinalize = 17,  // ... in the epilogue of a read -- sum
  kCtCycRead = 18,      // ... in a whole read -- sum
  kCtProblems = 22,     // distinct likelihood problems = positions of rep_list handed out, in chunks -- sum
  kCtLongReads = 25,    // entries of long_list (reads of several segments, set aside by the first accumulate launch) -- lane
  kCtStackSpills = 26,  // work stacks that outgrew the LDS: kr_timing.stack_spills -- sum
  kCtRows = 27,         // output rows (rows_mode) -- lane
  kCtTileHoles = 28,    // records of tiles that became holes (tiled batches) -- sum
  // KR_DEBUG_SKIP=512: path witnesses of the accumulate kernel (kr_debug_acc_paths; tests/test_gpu_acc_paths.py), one count by lane 0
  // where the path is entered -- all sum.  finalize_events_fast:
  kCtFpEntered = 29,        // calls
  kCtFpFalseEarly = 30,     // returned false at once: no events, or a threshold other than 4 (these two counted by process_read)
  kCtFpCompact = 31,        // compaction entered (events spilled, or more keys than one batch behind the events)
  kCtFpFalseCompacted = 32, // returned false after the compaction (the live events fill the LDS without overflowing it)
  kCtFpBigRead = 33,        // finish_big_read
  kCtFpOneBatch = 34,       // finished in one key batch
  kCtFpMultiBatch = 35,     // finished in several key batches
  kCtFpExtraBatches = 36,   // ... key batches beyond the first
  kCtFpDupCalls = 37,       // fix_dup calls
  kCtFpDupMoved = 38,       // ... that moved the count to another event
  // finalize_events:
  kCtGeEntered1 = 39,       // calls with events, one-segment instantiation
  kCtGeEntered2 = 40,       // ... two-segment instantiation (PB = 8)
  kCtGeEnteredMerge = 41,   // ... merge instantiation (once per segment)
  kCtGeFused = 42,          // planes filled while the ordinals are computed
  kCtGeSparse = 43,         // planes for the keys with several events only
  kCtGeBig = 44,            // planes in global scratch
  kCtGeExtraBatches = 45,   // key batches beyond the first
  kCtGeKeytabGlobal = 46,   // key table in global scratch
  kCtGeNoFit = 47,          // returned false: the read does not fit
  // process_read:
  kCtRdSetAside = 48,       // reads put on long_list by the one-segment launch
  kCtRdPlaneRedo = 49,      // reads done again with the plane tables (merge instantiation)
  kCtCount = 50
};
constexpr uint32_t kCtPathFirst = kCtFpEntered, kCtPathCount = kCtCount - kCtFpEntered;
constexpr uint32_t kCounterWords = (kCtCount + 31u) & ~31u; // words allocated, cleared and copied per lane: whole 128-byte lines
// Sets of BatchOut::cursors (kCursors * kCursorStride words each, kr_dev_scan.inc): every launch that hands out reads has its own
enum CursorSet : uint32_t { kCurScan = 0, kCurAcc1 = 1 /* one segment */, kCurAccMerge = 2 /* several */, kCurAcc2 = 3 /* two segments */, kCurSets = 4 };

// Everything the kernels write for one batch.
struct BatchOut {
  uint32_t* counters;    // [kCounterWords] indexed by CounterSlot
  uint32_t* cursors;     // read cursors of the scan and the accumulate launches, [kCurSets][kCursors * kCursorStride]
  uint32_t* rd_off;
  uint32_t* rd_cnt;
  uint32_t* rd_onmers;
  uint32_t* rd_filt;     // [2*nreads] raw per-strand hdist_filt (tap)
  uint8_t* rd_na;
  uint32_t* rec_read;
  uint32_t* rec_key;
  uint32_t* rec_hist;    // [np][rec_stride]: hist[x] of record i at x * rec_stride + i (coalesced across records)
  double* rec_d;
  double* rec_v;
  double* rec_chisq;
  uint8_t* rec_sel;
  // likelihood de-duplication (kr_dedup_kernel): records with the same (leaf, histogram, #k-mers) are one problem
  uint64_t* rec_w0;      // [rec_cap] the record's likelihood problem packed in one word by kr_acc_kernel (0: not packable):
                         // five 8-bit counts, the read's k-mer count in bits 40..55, bit 63.  A record with a word has NO
                         // histogram planes and no rec_read entry unless hist_always is set: the word says it all
  uint32_t hist_always;  // this batch keeps every record's planes (KR_TAP_ACCS: taps, `place`)
  uint32_t keep_v;       // rec_v is wanted (not a rows-only batch: KR_ROWS_ONLY without taps and without --filter needs DIST alone)
  uint32_t* rec_rep;     // [rec_cap] position of the record's representative in rep_list (0xFFFFFFFF: hole)
  uint32_t* rep_list;    // [rec_cap] record index of every distinct problem
  double2* rep_dv;       // [rec_cap] (d_llh, v_llh) per distinct problem
  uint32_t rep_cap;      // positions rep_list / rep_dv hold for this launch (rec_cap + kRepSlack; less in tests: KR_DEBUG_LIST_CAPS): a batch that
                         // hands out more -- its waves leave the tails of their chunks unused -- raises kErrRecCap instead of writing past the lane's slice
  ulonglong2* dd_table;  // [dd_slots] open-addressing table: x = histogram word (0 = empty), y = leaf | (list position + 1) << 32
  // Direct-mapped part (round 5): a record whose histogram counts at most kDdMaxEvents events -- 80 % of all records -- needs no
  // table probe: its problem is (onmers slot, class of the histogram, leaf) and dd_direct[(slot * kDdClasses + class) * dd_nodes + se]
  // is its place; the record stores its index there (a plain store: any of the equal records serves as representative),
  // kr_dedup_direct_kernel turns the marked places into list positions, the select kernels look the position up.
  uint32_t* dd_direct;   // [kDdOslots * kDdClasses * dd_nodes] 0xFFFFFFFF = unused this batch, else record index, later list position
  double2* dd_dv;        // [as dd_direct] (d_llh, v_llh) of the place's problem, copied from rep_dv by kr_dedup_dv_kernel: a select kernel
                         // reads a direct record's value with ONE look-up (place -> value) instead of two in a row (place -> position -> value)
  uint32_t* dd_ohist;    // [256 + 1] reads per k-mer count (records' onmers), the blocks' ticket
  uint8_t* dd_oslot;     // [256] k-mer count -> slot (0xFF: none): the kDdOslots most frequent counts of the batch
  const uint8_t* dd_cls; // [1024] c0 | c1 << 2 | c2 << 4 | c3 << 6 | c4 << 8 (counts <= 3) -> class, 0xFF if the sum is 0 or above kDdMaxEvents
  uint32_t dd_nodes;     // tree_nnodes + 1 (0: no direct part)
  uint32_t dd_slots;     // power of two
  uint32_t dd_shift;     // slots used per batch = records >> dd_shift (rounded up to a power of two)
  uint32_t rec_cap;      // record slots of this launch (a lane's slice of the stream's record arrays)
  uint64_t rec_stride;   // distance between the histogram planes = record slots of the whole stream
  kr_hit* hits;
  uint32_t hit_cap;
  // scan kernel -> accumulate kernel: resolved hits (colour, tag) of every read, contiguous per read
  uint2* items;          // x = entry index (low 32), y = pos(7) | strand<<7 | lib(4)<<8 | hd(5)<<12 | index high(8)<<17;
                         // y bit 31: segment marker, x = segment number
                         // filter slots (format 9): y = pos(7) | strand<<7 | lib(4)<<8 | hd12(3)<<12 | query rest bits(8)<<15 |
                         // index high(8)<<23, x = low 32 bits of the sx index; hd12 = 7: a verified entry of the PACKED arrays
                         // (bucket tail beyond 80 entries), hd in bits 15..19, x | high = packed entry index
  const uint8_t* v_tile; // [nreads] tiled batch (kr_dev_tiles.inc): 1 = this read is a tile of a long sequence; else null
  // Rows-only batches (KR_ROWS_ONLY): the output rows leave the device COMPACT -- (key, DIST) of the selected records only, a
  // read's rows contiguous -- instead of every record slot with a selection flag (kr_rows_* kernels, kr_dev_likelihood.inc)
  uint32_t rows_mode;    // the select kernels count every read's rows into rd_rcnt
  uint32_t* rd_rcnt;     // [nreads] rows of the read
  uint32_t* rd_roff;     // [nreads] its first row in row_key / row_d
  uint32_t* row_bsum;    // [ceil(nreads / kRowBlock) + 1] rows per block of reads, then (in place) the blocks' first rows
  uint32_t* row_key;     // [rec_cap] aliases rec_rep (dead once the select kernel has run)
  double* row_d;         // [rec_cap] aliases rep_dv (likewise)
                         // (tiled batches submitted with KR_TILE_ROWS use the two as well: what runs behind the select kernels there --
                         //  kr_tile_gather_kernel, per-read arrays only; kr_rebase_kernel never, a tiled batch is one lane -- reads neither)
  // KR_ROWS_INDEXED (one-lane batches): a row is (key, position of its DIST in the batch's list of distinct problems): 8 bytes
  // across PCIe instead of 12.  The row kernel reads rec_rep then, so its two arrays alias rec_d (which it no longer reads; the
  // select kernels, which do, are done), and dist_list -- rep_dv's d_llh column, dense -- aliases rec_v (not written in a
  // rows-only batch)
  uint32_t rows_indexed;
  uint32_t* row_dix;     // [rec_cap]
  double* dist_list;     // [min(counters[kCtProblems], dist_cap)]
  uint32_t dist_cap;     // entries dist_list holds (rec_cap: it aliases rec_v; less in tests: KR_DEBUG_LIST_CAPS).  List positions are handed out
                         // up to rep_cap, which is more: a batch whose positions reach beyond dist_cap is run again with rec_d (kr_batch_wait)
  uint32_t item_cap;
  uint32_t* rd_it_off;
  uint32_t* rd_it_cnt;
  uint32_t rec_chunk;    // record slots a wave takes at a time: kRecChunk for large batches; small ones take less (every
                         // resident wave leaves a partly used chunk behind, and the host copies slots, not records)
  uint32_t* long_list;   // [max_reads] reads of several segments, set aside by the first accumulate launch (counters[kCtLongReads])
  // level-2 accumulator scratch, one region per resident wave
  uint32_t* g_planes; // [nwaves][nslots2][np][4]
  uint32_t* g_counts; // [nwaves][nslots2][np]
  uint32_t* g_list;   // [nwaves][nslots2]
  uint64_t* stk_spill; // [nwaves][kStackSpill] lower part of a work stack that outgrew the LDS (large clades)
  uint32_t nslots2;   // 2 * nleaves
  uint32_t g_list_words; // per wave: max(nslots2, ev_spill + tab_spill * (hist words + 1))
  uint32_t ev_spill, tab_spill, kt_spill; // event-mode spill capacities per wave (events, table entries, keys)
  uint32_t bm_words;  // ceil(nslots2 / 32)
};

enum : uint32_t { kErrRecCap = 1u, kErrStack = 2u, kErrTable = 4u, kErrHitCap = 8u, kErrItemCap = 16u };

struct BatchIn {
  const uint8_t* bases;
  const uint64_t* offsets;
  uint32_t nreads;
};

// ---------------------------------------------------------------------------
// Device helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

// LDS pointers carry their address space in the type so that every access is a ds_ instruction
// (a generic pointer that the compiler cannot trace back to LDS becomes a flat_ access, which
// waits on both the LDS and the vector-memory counters).
#define KR_LDS __attribute__((address_space(3)))
typedef KR_LDS uint32_t lds_u32;
typedef KR_LDS uint64_t lds_u64;
typedef KR_LDS uint16_t lds_u16;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t lds_cas(lds_u32* p, uint32_t expected, uint32_t desired)
{
  __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  return expected;
}
__device__ __forceinline__ void lds_or(lds_u32* p, uint32_t v) { __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ uint32_t lds_ld(lds_u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// The probe kernel runs one wave64 per workgroup, so LDS hand-offs are between lanes of ONE wave:
// LDS operations of a wave execute in issue order, and all that is needed is that the compiler
// keeps that order.  __syncthreads() would also drain every outstanding global load
// (s_waitcnt vmcnt(0)) and so serialise the prefetched bucket loads behind each LDS exchange.
#define WAVE_SYNC()                                          \
  do {                                                       \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
    __builtin_amdgcn_wave_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
  } while (0)

// filter slots: hd on the 12 positions of a 24-bit code (bits above 23 of either operand may hold anything), and on the 4 rest positions
__device__ __forceinline__ uint32_t hd_code24(uint32_t c, uint32_t q)
{
  const uint32_t z = c ^ q;
  return __popc((z | (z >> 12)) & 0xFFFu);
}
__device__ __forceinline__ uint32_t hd_rest8(uint32_t a, uint32_t b)
{
  const uint32_t z = a ^ b;
  return __popc((z | (z >> 4)) & 0xFu);
}
// hd = number of non-LSH positions that differ (popcount_lr32, src/common.hpp:175)
__device__ __forceinline__ uint32_t hd_lr32(uint32_t a, uint32_t b)
{
  uint32_t z = a ^ b, f;
#ifdef KR_NO_SDWA
  return __popc((z | (z >> 16)) & 0xFFFFu);
#endif
  // (z | z >> 16) & 0xffff in one instruction: OR of the two 16-bit halves, zero-extended (SDWA operand selects)
  asm("v_or_b32_sdwa %0, %1, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1" : "=v"(f) : "v"(z));
  return __popc(f);
}

__device__ __forceinline__ uint32_t hash_key(uint32_t key) { return key * 0x9E3779B1u; }

// Per-(k-mer, strand) front end shared by the probe kernel and the debug tap.
struct FrontEnd {
  uint32_t rix[2], enc32[2]; // [strand]
  bool valid;
};

// Three 64-bit ballots per bit array cover 192 bases of the segment; position j's window
// is bits [j, j+k) in read order.
struct SegBits {
  uint64_t L[3], H[3], N[3];
};

__device__ __forceinline__ void load_segment(const uint8_t* seq, uint64_t len, uint64_t base0, SegBits& sb)
{
  uint32_t lane = lane_id();
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    uint64_t bi = base0 + 64u * p + lane;
    uint32_t code = 4;
    if (bi < len) code = base_code(seq[bi]);
    sb.L[p] = __ballot(code & 1u && code < 4);
    sb.H[p] = __ballot((code >> 1) & 1u && code < 4);
    sb.N[p] = __ballot(code >= 4);
  }
}

__device__ __forceinline__ uint32_t window32(uint64_t w0, uint64_t w1, uint32_t s)
{
  uint64_t v = s ? ((w0 >> s) | (w1 << (64 - s))) : w0;
  return (uint32_t)v;
}

// Position j = 64*pp + lane of the segment; (l0, l1), (h0, h1), (n0, n1) are the 64-bit words pp and pp + 1 of the three
// bit strings.
__device__ __forceinline__ FrontEnd front_end_words(const DevIndex& ix, uint64_t l0, uint64_t l1, uint64_t h0, uint64_t h1, uint64_t n0,
                                                    uint64_t n1, uint32_t j, uint32_t npos_seg)
{
  FrontEnd fe;
  const uint32_t lane = lane_id();
  uint32_t mk = (1u << ix.k) - 1u;
  uint32_t wl = window32(l0, l1, lane) & mk;
  uint32_t wh = window32(h0, h1, lane) & mk;
  uint32_t wn = window32(n0, n1, lane) & mk;
  fe.valid = (wn == 0) && (j < npos_seg);
  // position p of the k-mer counts from its LAST base (SURVEY.md Appendix C)
  uint32_t lo_f = __brev(wl) >> (32 - ix.k), hi_f = __brev(wh) >> (32 - ix.k);
  uint32_t lo_r = ~wl & mk, hi_r = ~wh & mk; // reverse complement: complement, order already reversed
  fe.rix[0] = spread16(pext32(lo_f, ix.pmask)) | (spread16(pext32(hi_f, ix.pmask)) << 1);
  fe.rix[1] = spread16(pext32(lo_r, ix.pmask)) | (spread16(pext32(hi_r, ix.pmask)) << 1);
  fe.enc32[0] = pext32(lo_f, ix.nmask) | (pext32(hi_f, ix.nmask) << 16);
  fe.enc32[1] = pext32(lo_r, ix.nmask) | (pext32(hi_r, ix.nmask) << 16);
  return fe;
}
// pp = 0/1 known at compile time (the caller's loop is unrolled: SegBits stays in scalar registers)
__device__ __forceinline__ FrontEnd front_end(const DevIndex& ix, const SegBits& sb, int pp, uint32_t npos_seg)
{
  return front_end_words(ix, sb.L[pp], sb.L[pp + 1], sb.H[pp], sb.H[pp + 1], sb.N[pp], sb.N[pp + 1], 64u * pp + lane_id(), npos_seg);
}
// pp = 0/1 wave-uniform at run time: scalar selects (indexing the arrays would put them in scratch memory)
__device__ __forceinline__ FrontEnd front_end_sel(const DevIndex& ix, const SegBits& sb, uint32_t pp, uint32_t npos_seg)
{
  const bool p1 = pp != 0;
  return front_end_words(ix, p1 ? sb.L[1] : sb.L[0], p1 ? sb.L[2] : sb.L[1], p1 ? sb.H[1] : sb.H[0], p1 ? sb.H[2] : sb.H[1],
                         p1 ? sb.N[1] : sb.N[0], p1 ? sb.N[2] : sb.N[1], 64u * pp + lane_id(), npos_seg);
}

// ---------------------------------------------------------------------------
// The same front end from BYTE TABLES in LDS (round 4; the slotted scan kernels, which are bound by instruction issue: eight
// software PEXTs + four bit spreads per position pair were 230 of their ~1,500 instructions per group of 64 positions).
// x86's PEXT (src/lshf.cpp:62-69) moves the bits at a fixed set of positions; for one BYTE of the k-bit window that is a
// function of 256 values, so four tables of 256 entries hold, for byte b of the window word (bit i = the base at read
// position j + i), everything that byte contributes to
//    .x  the forward strand's row-id half   (position p = k-1-i counts from the k-mer's last base; bit 2t if p = pasc[t])
//    .y  the forward strand's residual half (bit t if p = nasc[t])
//    .z  the reverse strand's row-id half   (position p = i: complement, order reversed; the complement is taken afterwards)
//    .w  the reverse strand's residual half
// already spread and shifted into place: a half is the OR of its word's four entries, bits at i >= k contribute nothing (no
// masking of the window), and one ds_read_b128 per byte serves both strands: 8 LDS reads + ~30 vector instructions per
// position pair.  The tables (16 KB) are built on the host at upload (kr_host_index.inc: build_fe_tab) and copied into LDS by
// every workgroup at its start.  Bit-exact with front_end_words (tests/test_gpu_parity.py::test_front_end_bit_exact runs all three).
// ---------------------------------------------------------------------------
typedef KR_LDS u32x4 lds_u32x4;
__device__ __forceinline__ void fe_tab_to_lds(const DevIndex& ix, lds_u32x4* tab)
{ // (whole workgroup; the caller synchronises)
  for (uint32_t i = threadIdx.x; i < 1024u; i += blockDim.x) {
    const uint4 v = ix.fe_tab[i];
    tab[i] = u32x4{v.x, v.y, v.z, v.w};
  }
}
__device__ __forceinline__ u32x4 fe_tab_word(const lds_u32x4* tab, uint32_t w)
{ // OR of the four byte entries of window word w (entry address = table b + byte b of w, 16 bytes each: one SDWA shift per byte)
  uint32_t a0, a1, a2, a3;
  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(a0) : "v"(4u), "v"(w));
  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(a1) : "v"(4u), "v"(w));
  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(a2) : "v"(4u), "v"(w));
  asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(a3) : "v"(4u), "v"(w));
  const KR_LDS uint8_t* base = (const KR_LDS uint8_t*)tab;
  const u32x4 e0 = *(const lds_u32x4*)(base + a0), e1 = *(const lds_u32x4*)(base + 4096u + a1), e2 = *(const lds_u32x4*)(base + 8192u + a2),
              e3 = *(const lds_u32x4*)(base + 12288u + a3);
  return (e0 | e1) | (e2 | e3);
}
__device__ __forceinline__ FrontEnd front_end_tab(const DevIndex& ix, const lds_u32x4* tab, uint64_t l0, uint64_t l1, uint64_t h0, uint64_t h1,
                                                  uint64_t n0, uint64_t n1, uint32_t j, uint32_t npos_seg)
{
  FrontEnd fe;
  const uint32_t lane = lane_id();
  const uint32_t mk = (1u << ix.k) - 1u;
  const uint32_t wl = window32(l0, l1, lane), wh = window32(h0, h1, lane), wn = window32(n0, n1, lane) & mk;
  fe.valid = (wn == 0) && (j < npos_seg);
  const u32x4 lo = fe_tab_word(tab, wl), hi = fe_tab_word(tab, wh);
  const uint32_t pm = (1u << (2u * ix.h)) - 1u, nm = ((1u << (ix.k - ix.h)) - 1u) * 0x10001u;
  fe.rix[0] = lo.x | (hi.x << 1);
  fe.enc32[0] = lo.y | (hi.y << 16);
  fe.rix[1] = ~(lo.z | (hi.z << 1)) & pm; // the reverse strand reads the complemented bases
  fe.enc32[1] = ~(lo.w | (hi.w << 16)) & nm;
  return fe;
}
__device__ __forceinline__ FrontEnd front_end_tab_sel(const DevIndex& ix, const lds_u32x4* tab, const SegBits& sb, uint32_t pp, uint32_t npos_seg)
{
  const bool p1 = pp != 0;
  return front_end_tab(ix, tab, p1 ? sb.L[1] : sb.L[0], p1 ? sb.L[2] : sb.L[1], p1 ? sb.H[1] : sb.H[0], p1 ? sb.H[2] : sb.H[1],
                       p1 ? sb.N[1] : sb.N[0], p1 ? sb.N[2] : sb.N[1], 64u * pp + lane_id(), npos_seg);
}

// ---------------------------------------------------------------------------
// The same front end from BIT PLANES (the slotted scan kernels: they are bound by VALU issue, and eight software PEXTs per
// position pair were a third of their instructions).  Lane i of a group handles position j0 + i, so bit t of its row id is
// bit (j0 + i + const) of the segment's bit string L or H: for all 64 lanes at once that is a 64-bit WINDOW of the string --
// a wave-uniform value made by two scalar shifts -- and the lane takes its bit as the carry-in of  acc = acc + acc + carry
// (v_addc_co_u32 with the window as the carry mask): ONE vector instruction per bit of rix / enc32, 4 * k per position pair,
// the windows on the scalar unit.  Validity (no N in the k-mer, position within the segment) is a wave-uniform mask too.
// Bit-exact with front_end_words (tests/test_gpu_parity.py::test_front_end_bit_exact runs both).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t plane_window(uint64_t a, uint64_t b1, uint32_t t)
{ // bits [t, t + 64) of the string whose first word is a and whose second word, shifted left by one, is b1; t < 64; wave-uniform
  return (a >> t) | (b1 << (63u - t));
}
__device__ __forceinline__ uint32_t shl1_add_bit(uint32_t acc, uint64_t plane)
{ // 2 * acc + bit `lane` of the wave-uniform mask
  uint32_t r;
  uint64_t co;
  asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(r), "=s"(co) : "v"(acc), "s"(plane));
  return r;
}
struct PlaneFe {
  uint32_t rix[2], enc32[2]; // [strand]
  uint64_t valid;            // wave-uniform: bit i = position j0 + i holds a valid k-mer
};
__device__ __forceinline__ PlaneFe front_end_planes(const DevIndex& ix, const SegBits& sb, uint32_t pp, uint32_t npos_seg)
{
  PlaneFe fe;
  const uint32_t j0 = 64u * pp, k = ix.k, h = ix.h, nn = k - h;
  // the 128 bits of every string from position j0 on (every shift below is < k <= 31)
  const uint64_t La = pp ? sb.L[1] : sb.L[0], Lb = (pp ? sb.L[2] : sb.L[1]) << 1;
  const uint64_t Ha = pp ? sb.H[1] : sb.H[0], Hb = (pp ? sb.H[2] : sb.H[1]) << 1;
  // ---- validity: OR of the N string over the shifts 0 .. k-1 by doubling (c = largest power of two <= k: smear_c | smear_c >> (k - c))
  {
    uint64_t lo = pp ? sb.N[1] : sb.N[0], hi = pp ? sb.N[2] : sb.N[1];
    uint32_t c = 1;
#pragma unroll
    for (uint32_t st = 1; st <= 8u; st <<= 1) {
      if (2u * st <= k) {
        lo |= (lo >> st) | (hi << (64u - st));
        hi |= hi >> st;
        c = 2u * st;
      }
    }
    const uint32_t rest = k - c; // < c
    const uint64_t sm = lo | (lo >> rest) | ((hi << 1) << (63u - rest));
    const uint32_t left = npos_seg > j0 ? npos_seg - j0 : 0u;
    fe.valid = ~sm & (left >= 64u ? ~0ull : ((1ull << left) - 1ull));
  }
  // ---- row ids: bit 2t = low bit, 2t + 1 = high bit of the base at LSH position pasc[t]; MSB first.  Forward strand: position p
  //      counts from the k-mer's last base (shift k - 1 - p); reverse strand: complemented, order reversed (shift p)
  uint32_t rf = 0, rr = 0;
  {
    uint64_t w = ix.ppk[0];
    for (uint32_t t = 0; t < h; ++t) {
      if (t == 12u) w = ix.ppk[1];
      const uint32_t p = (uint32_t)w & 31u, sf = k - 1u - p;
      w >>= 5;
      rf = shl1_add_bit(rf, plane_window(Ha, Hb, sf));
      rf = shl1_add_bit(rf, plane_window(La, Lb, sf));
      rr = shl1_add_bit(rr, ~plane_window(Ha, Hb, p));
      rr = shl1_add_bit(rr, ~plane_window(La, Lb, p));
    }
  }
  fe.rix[0] = rf, fe.rix[1] = rr;
  // ---- residual codes: bit t = low bit, 16 + t = high bit at non-LSH position nasc[t] (zero-padded to 16)
  uint32_t ef = 0, er = 0;
  {
    uint64_t w = ix.npk[0];
    for (uint32_t t = 0; t < nn; ++t) {
      if (t == 12u) w = ix.npk[1];
      const uint32_t p = (uint32_t)w & 31u;
      w >>= 5;
      ef = shl1_add_bit(ef, plane_window(Ha, Hb, k - 1u - p));
      er = shl1_add_bit(er, ~plane_window(Ha, Hb, p));
    }
    ef <<= 16u - nn, er <<= 16u - nn;
    w = ix.npk[0];
    for (uint32_t t = 0; t < nn; ++t) {
      if (t == 12u) w = ix.npk[1];
      const uint32_t p = (uint32_t)w & 31u;
      w >>= 5;
      ef = shl1_add_bit(ef, plane_window(La, Lb, k - 1u - p));
      er = shl1_add_bit(er, ~plane_window(La, Lb, p));
    }
  }
  fe.enc32[0] = ef, fe.enc32[1] = er;
  return fe;
}

// Index::check_partial + Index::bucket_indices (src/index.hpp:27, src/index.cpp:160-168)
template <bool SL>
__device__ __forceinline__ bool locate_row(const DevIndex& ix, uint32_t rix, int& lib, uint32_t& row)
{
  uint32_t res, q;
  if (ix.m_shift != 0xFFFFFFFFu) {
    res = rix & (ix.m - 1u);
    q = rix >> ix.m_shift;
  } else {
    q = rix / ix.m;
    res = rix - q * ix.m;
  }
  uint32_t numer, nrows;
  if (SL) { // everything from kernel arguments
    if (!((ix.res_mask >> res) & 1ull)) return false;
    lib = 0;
    numer = ix.lib0.numer;
    nrows = ix.lib0.nrows;
  } else {
    lib = ix.res_lib[res];
    if (lib < 0) return false;
    numer = ix.libs[lib].numer;
    nrows = ix.libs[lib].nrows;
  }
  row = numer > 1 ? q * numer + res : q;
  return row < nrows;
}

// Loads / stores / atomics on a wave's own global scratch (event spill, key and record tables, level-2 planes and counts):
// written and read back by the same wave only, so workgroup scope orders them.  Agent scope sets sc1, which makes every such
// store write through the XCD's L2 to HBM and every load miss it (measured: 1.56 GB of the accumulate kernel's 2.34 GB
// WRITE_SIZE per 1 M reads); at workgroup scope the scratch lives in the L2 as write-back lines.
#ifndef KR_SCRATCH_SCOPE
#define KR_SCRATCH_SCOPE __HIP_MEMORY_SCOPE_WORKGROUP
#endif
__device__ __forceinline__ uint32_t gload(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, KR_SCRATCH_SCOPE); }
__device__ __forceinline__ void gstore(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, KR_SCRATCH_SCOPE); }

// Work-stack item (8 B): lo = tagged colour id, hi = pos(7) | strand(1)<<7 | lib(4)<<8 | hd(5)<<12.
// The items the scan kernel hands over name the table ENTRY instead (index low in lo, high 8 bits in hi
// bits 17..24); the accumulate kernel fetches the colour.
__device__ __forceinline__ uint32_t tag_pos(uint32_t t) { return t & 127u; }
__device__ __forceinline__ uint32_t tag_strand(uint32_t t) { return (t >> 7) & 1u; }
__device__ __forceinline__ uint32_t tag_lib(uint32_t t) { return (t >> 8) & 15u; }
__device__ __forceinline__ uint32_t tag_hd(uint32_t t) { return (t >> 12) & 31u; }

// SL (single library, m <= 64) is a compile-time property of the launched kernel: the library
// descriptor and the residue mask then come from kernel arguments (SGPRs) with no load at all.
template <bool SL>
__device__ __forceinline__ DevLib get_lib(const DevIndex& ix, uint32_t lib)
{
  if (SL) return ix.lib0;
  return ix.libs[lib];
}

// Colour ids in HBM carry their class in the top two bits (set once at upload, see
// colour_classes in kr_host_index.inc): 0 = drop (empty set / null tree node), 1 = tree leaf (low bits = leaf RANK, the
// index among leaves in colour-id order), 2 = expand through se_to_pse (low bits = colour id), 3 = FLAT (low bits = colour
// id; its se_to_pse slot holds {base, count} instead of the two parts): a colour whose leaves are known at upload -- a run
// of `count` consecutive ranks from `base` (every clade of the tree: ranks follow the post-order numbering), or, with bit 31
// of `base` set, `count` <= kFlatMax ranks listed at leaflist[base ...] (every other small colour).  A flat colour costs
// one gather (two for a list) and no walk: the breadth-first expansion of src/query.cpp:369-387 visits 2 * cardinality - 1
// colours level by dependent level, and the colours the builder makes by merging up the tree are chains as deep as they
// have leaves -- ONE deep colour among a read's hits kept the whole wave stepping (5.8 drain steps per read at 13 of 64
// lanes busy on the 1000-genome index, before).  Only large scattered colours are still walked (class 2).
// This replaces Tree::check_node + get_node + check_leaf (src/query.cpp:371-381) and a dependent
// load per colour.
constexpr uint32_t kColMask = 0x3FFFFFFFu;

// Inclusive prefix sum over the wave on the DPP network (row shifts 1, 2, 4, 8, then the row totals broadcast into the
// following rows): six adds, against six LDS permutes with their address arithmetic for the __shfl_up form.
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v)
{
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false); // row_shr:1
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false); // row_shr:2
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false); // row_shr:4
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false); // row_shr:8
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false); // row_bcast:15 into rows 1 and 3
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false); // row_bcast:31 into rows 2 and 3
  return v;
}
// OR over the wave, same network (the result is wave-uniform: read from lane 63)
__device__ __forceinline__ uint32_t wave_or(uint32_t v)
{
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t lanes_below(uint64_t m)
{ // number of set bits of m below this lane
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
