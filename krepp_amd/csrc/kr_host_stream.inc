// kr_host_stream.inc -- part of kr_device.hip (host side): lanes, kr_stream_create / destroy, kr_batch_submit / wait / collect / timing.

// ---------------------------------------------------------------------------
// kr_stream
// ---------------------------------------------------------------------------
// One batch is cut into up to kMaxLanes contiguous read ranges ("lanes").  A lane is a complete pipeline of its own --
// HIP stream, H2D copy of its reads, the kernels, its counters -- working on its slice of the stream's result arrays,
// so that the copies of one lane and the kernels of another overlap, and the three kernel families (scan: HBM request
// rate; accumulate: latency; likelihood: fp64 ALU) of different lanes can share the chip.  Lanes change nothing in any
// result: reads are independent, and every lane runs the same kernels on its reads.
constexpr uint32_t kMaxLanes = 8;
enum LaneEvent { // Lane::ev; kr_batch_timing's intervals lie between them
  kEvCopyIn = 0,   // before the copies in
  kEvFirstKernel,  // before the lane's first kernel (behind the index's kernel chain)
  kEvScanDone,     // scan done
  kEvAccDone,      // accumulate done
  kEvLastKernel,   // behind the last kernel
  kEvAccStart,     // recorded right behind kEvScanDone: start of the accumulate stage
  kEvLlhStart,     // recorded right behind kEvAccDone: start of the likelihood stage
  kEvCount
};
struct Lane {
  hipStream_t stream = nullptr;
  hipEvent_t ev[kEvCount] = {}; // indexed by LaneEvent
  BatchIn in;
  BatchOut out;                // pointers: the lane's private scratch + its slices of the stream's arrays
  uint32_t* d_counters = nullptr;
  uint32_t* d_cursors = nullptr;
  ulonglong2* d_dd = nullptr;  // private de-duplication table
  uint32_t dd_slots = 0;
  uint32_t* d_dd_direct = nullptr; // ... its direct-mapped part, the k-mer-count histogram and slots
  double2* d_dd_dv = nullptr;      // ... the values of its places
  uint32_t* d_dd_ohist = nullptr;
  uint8_t* d_dd_oslot = nullptr;
  uint32_t *d_g_planes = nullptr, *d_g_counts = nullptr, *d_g_list = nullptr;
  uint64_t* d_stk = nullptr;
  uint32_t* h_counters = nullptr; // pinned [kCounterWords]
  // this batch
  uint32_t read0 = 0, nreads = 0, rec_base = 0, rec_cap = 0, nrecs = 0;
  uint32_t nrows = 0;          // rows-mode batches: output rows of the lane (counters[kCtRows])
  uint64_t host_off = 0;       // where the lane's records (rows) start in the compacted host arrays
};

// The batch in flight (docs/design/08, "The batch in flight").  BatchOrigin: what the caller of the internal submit knows about the
// batch and hands in; the reruns of kr_batch_wait submit again from the record of the batch they rerun, one mode bit changed.
enum IdSource : uint8_t { kIdsNone, kIdsHost, kIdsDevice }; // no ids; staged in text.h_ids by kr_batch_submit_text; written into text.d_ids by a record finder
struct BatchOrigin {
  IdSource ids = kIdsNone;
  uint64_t id_bytes = 0;
  uint32_t id_sep = 0;
  bool parsed = false;    // a record finder produced the batch (kr_batch_submit_fastq / _fasta / _bgzf): bases, offsets and names are the device's
  bool untiled = false;   // (rerun) a tiled batch that overflowed a device buffer: one wave per sequence this time
  bool unindexed = false; // (rerun) an indexed batch whose list positions outgrew dist_list: KR_ROWS_INDEXED is ignored this time
};
// Everything that is true of the batch in flight and of nothing else.  begin_batch assigns a fresh one: what nobody sets is at its default
struct Batch {
  bool submitted = false, waited = false, collected = false;
  int rc = 0; // result of the batch, returned by every wait / collect until the next submit (errors are sticky)
  std::string msg;
  const uint8_t* bases = nullptr; // the arguments of the submit (host buffers stay valid until wait / collect returns)
  const uint64_t* offsets = nullptr;
  uint32_t nreads = 0, flags = 0;
  BatchOrigin from;
  uint32_t nlanes = 0;
  bool tiled = false;           // submitted as tiles: `nreads` real reads, `nv` reads on the device, `nlong` long sequences among them
  bool tiles_on_device = false; // ... and the Tiles' d_ arrays were filled by the kr_tile_lay_* kernels (no h_ array holds anything of it)
  uint32_t nv = 0, nlong = 0;
  bool rows_mode = false;    // leaves the device as compact rows (KR_ROWS_ONLY, no taps; tiled: with KR_TILE_ROWS)
  bool rows_indexed = false; // ... of 8 bytes: (key, index into the batch's distinct DIST values) -- KR_ROWS_INDEXED
  bool text_made = false;    // submitted with ids, and its text kernels were queued
  bool seek = false;         // a seek batch (kr_host_seek.inc)
  bool seek_view = false;    // ... whose values are in the page-locked mirrors
  bool extract = false;      // ... whose reads the extract kernels split (kr_host_extract.inc): a record finder queued it on an extract stream
  uint32_t extract_have = 0; // ... and the parts (KR_EXTRACT_*) that are in the page-locked mirror
  bool extract_deferred = false; // ... or would have, on a stream with kr_stream_extract_defer: kr_batch_extract_pair queues the kernels
  uint32_t nrecs = 0;
  uint64_t nhits = 0;
  uint64_t ndist = 0, h_ndist = 0; // entries of the batch's list of distinct values (set by kr_batch_wait: a device view shows it too), of its host copy
  bool has_ids() const { return from.ids != kIdsNone; }
};
// The last call of a record finder on the stream: not every one queues a batch (zero bytes, zero accepted records, a rejected BGZF
// member), and its names can be asked for either way.  A batch that no record finder produced ends it.
struct LastParse {
  bool parsed = false;     // the last submit on the stream was kr_batch_submit_fastq / _fasta / _bgzf: its names can be asked for
  bool have_names = false; // ... and they are in Fastq::name_pos / h_nlen
  uint32_t nreads = 0;
};

struct kr_stream {
  const kr_index* ix = nullptr;
  int device = 0; // copy of ix->device: destroying a stream must not read an index that may already be gone
  kr_params params;
  DevParams dp;
  LlhConst llh;
  uint32_t max_reads = 0;
  uint64_t max_bases = 0;
  uint32_t rec_cap = 0, hit_cap = 0, item_cap = 0;
  uint64_t rec_user_cap = 0; // the caller's max_records (rec_cap adds per-wave chunk slack per lane)
  uint32_t nwaves = 0, nwaves_full = 0, nwaves_lean = 0, nwaves_lean2 = 0; // per-wave scratch slots; grids of the accumulate launches
  uint32_t max_lanes = 1; // lanes created (of the batch in flight: Batch::nlanes)
  uint32_t lane_min_reads = 1u << 16;
  bool lanes_for_device_input = false;
  Lane lanes[kMaxLanes];
  // device: input staging and the result arrays every lane writes its slice of
  uint8_t* d_bases = nullptr;
  uint64_t* d_offsets = nullptr; // [max_reads + max_lanes]: every lane has its own nreads + 1 entries
  BatchOut out;                  // the stream-wide arrays (and the constants every lane copies)
  // Who owns what: buffers that live as long as the stream are allocated by salloc / halloc into these two lists and freed in bulk
  // by kr_stream_destroy -- the lists are append-only, nothing is ever taken out of them; every buffer that grows with the batches
  // is a DevBuf / PinBuf (kr_buf.h) that frees itself; the structs handed to kernels hold raw pointers filled from get()
  std::vector<void*> dallocs;
  size_t nfresh = 0;             // device buffers made so far, the item lists included (KR_DEBUG_POISON=<k> names the k-th)
  DevBuf<uint2> items;           // out.items: the item list in use (ItemPlacement may exchange it for another)
  DevBuf<kr_hit> d_hits;         // out.hits, made by the first KR_TAP_HITS batch
  // pinned host
  uint8_t* h_bases = nullptr;
  uint64_t* h_offsets = nullptr;
  uint32_t h_counters[kCounterWords] = {0}; // the lanes' counters combined (kCounterRules)
  uint32_t *h_rd_off = nullptr, *h_rd_cnt = nullptr, *h_rd_onmers = nullptr, *h_rd_filt = nullptr;
  uint8_t* h_rd_na = nullptr;
  std::vector<void*> hallocs;
  // the records' host arrays grow on demand in kr_batch_collect (all of h_rec_key's size; hist: np times that)
  PinBuf<uint32_t> h_rec_key, h_rec_hist;
  PinBuf<uint8_t> h_rec_sel;
  PinBuf<double> h_rec_d, h_rec_v, h_rec_chisq;
  PinBuf<kr_hit> h_hits;
  // `place` back end on the device (kr::place_on_device): the placement tree as device arrays (for one tree at a
  // time), per-read / per-candidate outputs and their page-locked mirrors; grown on demand
  struct PlaceWs {
    const void* tree_tag = nullptr;
    uint32_t pn = 0, nidx = 0;
    DevBuf<uint32_t> d_parent, d_eff, d_lo, d_idx_to_pt, d_depth;
    uint32_t cu_count = 0;
    DevBuf<uint4> d_node; // {parent, lo, eff, depth} of every node: one 16-byte load per level of a walk up the tree
    DevBuf<double> d_chain; // per wave of kr_place_kernel: the weights of every (leaf, ancestor) pair of the read in hand
    uint32_t chain_cap = 0, chain_waves = 0;
    DevBuf<uint8_t> d_elig;
    DevBuf<uint32_t> d_len, d_c0, d_info; // per read: one capacity, with h_len / h_c0 / h_info
    DevBuf<uint32_t> d_cse, d_cread;      // per candidate slot: one capacity, with d_cd / d_cv / d_cchi
    DevBuf<uint32_t> d_cnt;
    DevBuf<double> d_cd, d_cv, d_cchi, d_cprob, d_rprob;
    DevBuf<uint32_t> d_kse; // the candidates that pass the chi-square test, compacted (kr_place_compact_kernel); one capacity with d_kd / d_kv / d_kchi
    DevBuf<double> d_kd, d_kv, d_kchi;
    uint64_t keep_want_min = 0; // what a batch that ran out of kept-candidate slots asked for
    DevBuf<uint32_t> d_heavy, d_heavy_u32; // reads beyond the LDS arrays of kr_place_kernel: their list, the second launch's scratch
    DevBuf<double> d_heavy_f64;
    uint32_t heavy_leaves = 0, heavy_nodes = 0, heavy_waves = 0;
    PinBuf<uint32_t> h_len, h_c0, h_info, h_cse, h_cnt; // (h_cse: one capacity with h_cd / h_cv / h_cchi)
    PinBuf<double> h_cd, h_cv, h_cchi;
    // rows as text on the device (round 6)
    const void* text_tree_tag = nullptr; // the tree whose branch lengths, subtree sizes and labels are uploaded
    DevBuf<double> d_blen;
    DevBuf<uint32_t> d_card, d_label_off;
    DevBuf<char> d_labels;
    bool text_on = false; // this batch's ranges are formatted on the device
    uint32_t text_tabular = 0, text_multi = 1;
    DevBuf<char> d_ids;
    PinBuf<char> h_ids;
    DevBuf<uint32_t> d_id_off;
    PinBuf<uint32_t> h_id_off;
    DevBuf<uint32_t> d_tlen;
    DevBuf<uint64_t> d_tbsum, d_ttotal;
    PinBuf<uint64_t> h_ttotal;
    DevBuf<char> d_text;
    PinBuf<char> h_text;
    uint64_t text_want_min = 0;
    // a batch the record finders queued (kr_place_stream_parsed; kr_dev_place_parsed.inc): the block sums of the names' lengths
    // and, page-locked, their total; ids_reads: reads whose ids the device laid out in d_ids / d_id_off for the last such call
    DevBuf<uint64_t> d_idbsum;
    PinBuf<uint64_t> h_idtot;
    uint32_t ids_reads = 0;
    bool ids_queued = false; // this batch's place_device_begin_parsed queued the id offsets and their total (want_ids)
    DevBuf<uint32_t> d_sse, d_rbest; // the kept candidates sorted by node (same slots as d_kse ...), per-read --no-multi choice
    DevBuf<double> d_sd, d_sv, d_sc, d_rtotal;
    // KR_DEBUG_PLACE_CAPS (tests; place_device_begin reads it per batch): what the kernels are told the candidate slots, the kept
    // slots and the text buffer hold, 0 = what they do hold; `dbg_sticky`: a range that is run again is given no more
    uint64_t dbg_cand = 0, dbg_keep = 0, dbg_text = 0, dbg_list = 0; // (dbg_list: entries of the kept slots the internal candidates' list may take)
    bool dbg_sticky = false;
  } pw;
  // Long sequences across waves (kr_dev_tiles.inc): a host batch with sequences of more than kTileMinPos k-mer positions
  // is submitted as a batch of tiles, and so is a batch in HBM submitted with KR_TILE_DEVICE.  Buffers are made on first use.
  struct Tiles {
    PinBuf<uint8_t> h_bases; // the tiled batch's bases (tiles overlap by k - 1); one capacity with d_bases
    DevBuf<uint8_t> d_bases;
    PinBuf<uint64_t> h_voff; // [max_reads + 1]
    DevBuf<uint64_t> d_voff;
    PinBuf<uint8_t> h_vtile; // [max_reads], as every array below (h_longs, d_longs and the two filt arrays: two words a read)
    DevBuf<uint8_t> d_vtile;
    PinBuf<uint32_t> h_rfirst, h_longs;
    DevBuf<uint32_t> d_rfirst, d_longs;
    DevBuf<uint32_t> d_tile_filt, d_real_off, d_real_cnt, d_real_onmers, d_real_filt;
    DevBuf<uint8_t> d_real_na;
    DevBuf<uint32_t> d_real_roff, d_real_rcnt; // a tiled rows-mode batch (KR_TILE_ROWS): the real reads' row ranges
    // the layout on the device: per-read scratch ([max_reads]), the block sums and the summary {nv, nlong, bases}
    DevBuf<uint8_t> d_choice;
    DevBuf<uint32_t> d_lread;
    DevBuf<uint64_t> d_vsrc, d_bsum, d_sum;
    PinBuf<uint64_t> h_sum;
  } tiles;
  std::vector<uint8_t> tile_choice; // per read of the batch in hand: submitted as tiles
  uint32_t tile_min_pos = kTileMinPos; // (KR_TILE_MIN_POS: experiments)
  std::vector<hipStream_t> moved_streams; // (kr_debug_stream_move: lane 0's earlier streams, destroyed with the stream)
  // Where the item list lies (DESIGN.md section 3.1b): the scan kernel's launch time depends on the physical pages behind the list
  // it writes (40.5 against 46.5 ms per 8 M reads, decided when the buffer is allocated), so a stream that is given large
  // batches tries a few allocations during its first batches and keeps the one its scan ran fastest on.
  struct ItemPlacement {
    int trials_left = -1;       // -1: KR_ITEM_PLACEMENT_TRIALS not read yet
    DevBuf<uint2> aside;        // the best list so far, set aside while another one is in use (exchanged with kr_stream::items)
    double best_ns = 0;         // its scan time per read
    uint32_t tried = 0, kept_new = 0;
    int settling = 2;           // launches of the list in use that are not measured yet: a list's first launch is ~6 ms slower than its
                                // later ones whatever list it is, and so is a process's second launch (profiles/round4_trials_*.txt):
                                // the stream's own list is measured at its third launch, a trial list at its second
  } ipl;
  // report text written on the device (kr_dev_text.inc; kr_stream_text_enable)
  struct Text {
    bool on = false;   // buffers exist
    char *d_ids = nullptr, *h_ids = nullptr;
    uint32_t *d_id_off = nullptr, *h_id_off = nullptr;
    uint64_t id_cap = 0;
    uint32_t* d_tlen = nullptr;
    uint64_t *d_bsum = nullptr, *d_total = nullptr, *h_total = nullptr;
    char* d_text = nullptr;
    PinBuf<char> h_text; // (made by the first batch that needs it, as large as that batch's text asks)
    uint64_t text_cap = 0;
    bool seek_only = false;     // the buffers were made by kr_stream_seek_enable: no node names are uploaded, `dist` text is not served
  } text;
  // `seek` on kernels of its own (kr_dev_seek.inc, kr_host_seek.inc; kr_stream_seek_enable).  A seek batch runs as one lane and uses
  // none of the item list, the record slots or the accumulate scratch
  struct Seek {
    bool on = false;
    uint32_t np = 0;
    uint32_t *d_first = nullptr, *d_bsum = nullptr; // [max_reads + 1], [max_reads / kRowBlock + 2]
    uint32_t* d_cnt = nullptr;                      // a batch's hist [nreads * 2 * np], then its onmers [nreads]
    double* d_d = nullptr;                          // a batch's d [nreads], then its d_strand [2 * nreads]
    uint32_t* h_cnt = nullptr;
    double* h_d = nullptr;
    hipEvent_t ev[4] = {}; // in front of the unit count, behind the hist kernel, behind the solve kernel, behind the text kernels
    bool timed = false;
  } seek;
  // FASTQ records found on the device (kr_dev_fastq.inc; kr_stream_fastq_enable)
  struct Fastq {
    bool on = false;
    uint64_t raw_cap = 0;             // bytes of a chunk
    uint8_t* d_raw = nullptr;         // [raw_cap rounded up to 16, + 16]
    uint32_t *d_tile_nl = nullptr, *d_nl = nullptr;
    uint32_t *d_slen = nullptr, *d_npos = nullptr, *d_nlen = nullptr, *d_id_off = nullptr;
    uint64_t *d_bsum_b = nullptr, *d_bsum_n = nullptr;
    unsigned long long* d_ctl = nullptr;
    kr_fastq_parse *d_sum = nullptr, *h_sum = nullptr;
    uint32_t *h_npos = nullptr, *h_nlen = nullptr;
    std::vector<uint64_t> name_pos;
    hipEvent_t ev_parse0 = nullptr, ev_parse1 = nullptr; // kr_debug_fastq_parse_ms: around the record finder's kernels, once asked for
    bool ev_set = false;
    // FASTA records (kr_dev_fasta.inc): made by the stream's first kr_batch_submit_fasta, sized from raw_cap and max_reads
    bool fa_on = false;
    uint32_t *d_tile_st = nullptr, *d_tile_gr = nullptr; // [tiles of raw_cap + 1]
    uint32_t *d_hs = nullptr, *d_ga = nullptr;           // [max_reads + 2]
    uint32_t *d_hg = nullptr, *d_he = nullptr;           // [max_reads]
    bool last_fasta = false; // the last chunk's records were found by the FASTA kernels (hs), not the FASTQ ones (nl)
  } fq;
  // block-gzipped chunks inflated into fq.d_raw (kr_dev_bgzf.inc; kr_stream_bgzf_enable)
  struct Bgzf {
    bool on = false;
    uint64_t comp_cap = 0;
    uint32_t max_members = 0;
    uint8_t *d_comp = nullptr, *d_scratch = nullptr; // [comp_cap], [2][65536]
    kr::BgzfMember *d_tab = nullptr, *h_tab = nullptr; // [max_members]
    uint32_t* d_status = nullptr;
    BgzfSum *d_sum = nullptr, *h_sum = nullptr;
    std::vector<uint64_t> member_off; // of the last chunk's members in `comp`, for the message of a rejected one
    hipEvent_t ev0 = nullptr, ev1 = nullptr; // kr_debug_bgzf_ms: around the inflate kernel, once asked for
    bool ev_set = false;
  } bgzf;
  // report text deflated into BGZF members on the device (kr_dev_deflate.inc, kr_host_deflate.inc; kr_stream_bgzf_out_enable)
  struct BgzfOut {
    bool on = false;
    DevBuf<uint8_t> d_slots, d_out, d_in; // [members][bgzf_slot_stride(member_in)], the members back to back, kr_debug_bgzf_deflate's bytes
    DevBuf<uint64_t> d_off;               // [members + 1]
    uint32_t level = 1;                   // kr_stream_bgzf_out_level: 1 fixed codes, 2 dynamic codes
    uint32_t member_in = kr::kDefMemberIn; // kr_stream_bgzf_member: input bytes of a member
    uint32_t place_level = 0;             // kr_stream_place_bgzf: 0 off; 1 / 2: kr_place_stream's text comes back as members
    DevBuf<uint32_t> d_tokens;            // level 2: [members][member_in], made when level 2 is first asked for
    DevBuf<uint32_t> d_huff;              // kr_debug_huffman_lengths_device: counts, lengths, the flag
    PinBuf<uint64_t> h_total;
    PinBuf<uint8_t> h_comp; // (made by the first batch that needs it, as large as that batch's text can become)
    hipEvent_t ev0 = nullptr, ev1 = nullptr; // kr_debug_bgzf_deflate_ms: around the three kernels, once asked for
    bool ev_set = false;
  } bgzf_out;
  // the reads of a seek batch split by their DIST on the device (kr_dev_extract.inc, kr_host_extract.inc; kr_stream_extract_enable)
  struct Extract {
    bool on = false;
    double max_dist = 0; // NaN: every read with a finite DIST is matched
    uint32_t *d_start = nullptr, *d_mpre = nullptr; // [max_reads + 1]
    uint64_t* d_bsum = nullptr;                     // [max_reads / kRowBlock + 2]
    uint8_t *d_out = nullptr, *h_out = nullptr;     // [raw_cap rounded up to 16, + 16]: matched bytes, then unmatched bytes
    unsigned long long *d_res = nullptr, *h_res = nullptr; // [4] matched bytes, matched records, records, consumed
    PinBuf<uint8_t> h_members; // kr_batch_collect_extract_bgzf: the matched part's members, then the unmatched part's
    hipEvent_t ev[2] = {};     // around the extract kernels
    bool timed = false;
    // paired reads (kr_stream_extract_defer, kr_batch_extract_pair): a seek submit leaves the split to the pair call
    bool defer = false;
    double* d_pair = nullptr;   // [max_reads] the pair values of the batch in flight, made by the first pair call
    hipEvent_t ev_x[2] = {};    // this stream's lane at the pair call (the other stream's lane waits for it); behind the pair call's last copy
  } extract;
  Batch batch;     // the batch in flight
  LastParse parse; // the last record finder's call
  // state
  bool h_rec_full = false; // the pinned record buffers hold v / chisq / hist only once a batch asked for them
  PinBuf<uint32_t> h_rec_dix; // of h_rec_key's size, allocated with the first indexed batch
  PinBuf<double> h_dist_list;
  uint64_t ix_extent = 0, ix_fallbacks = 0; // kr_debug_indexed_list: list positions of the last indexed launch, reruns so far
  uint64_t d2h_bytes = 0;    // what the last kr_batch_collect copied back
  uint64_t h_sel_ones = 0; // leading entries of h_rec_sel known to hold 1 (rows-mode views: every row is selected)
  uint32_t scan_blocks = 0, scan_pipe_blocks = 0, scan_filt_blocks = 0;
  bool scan_pipe = true; // slotted tables: the pipelined scan kernel (KR_SCAN_PIPE=0 when the stream was made: the one-group-at-a-time kernel)
  uint32_t item_cap_dbg = 0; // (tests) KR_DEBUG_ITEM_CAP when the stream was made: item slots a lane's scan is told its list holds (0: all of them)
  bool fk = false; // the index has filter slots (format 9) and this stream's threshold fits their candidates: kr_scan_filt_kernel_t + FK accumulate
};

namespace {

template <typename T>
int salloc(kr_stream* s, T** p, uint64_t n)
{
  HIP_TRY(hipMalloc((void**)p, std::max<uint64_t>(16, n * sizeof(T))));
  s->dallocs.push_back(*p);
  return poison_fresh(*p, std::max<uint64_t>(16, n * sizeof(T)), ++s->nfresh);
}
// An item list (kr_stream::items, or a trial's): counted and poisoned like the arena's buffers, owned by the caller's Buf
int new_item_list(kr_stream* s, DevBuf<uint2>& list)
{
  if (!list.renew(s->item_cap)) return alloc_failed("item list");
  return poison_fresh(list.get(), list.bytes(), ++s->nfresh);
}
template <typename T>
int halloc(kr_stream* s, T** p, uint64_t n)
{
  HIP_TRY(hipHostMalloc((void**)p, std::max<uint64_t>(16, n * sizeof(T)), hipHostMallocDefault));
  s->hallocs.push_back(*p);
  return KR_OK;
}

uint32_t next_pow2(uint32_t v)
{
  uint32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// KR_DEBUG_LIST_CAPS="dist,rep" (tests; read at every submit, as KR_DEBUG_PLACE_CAPS is per batch): what the kernels are told the list of
// distinct likelihood problems holds -- `dist` entries of dist_list (KR_ROWS_INDEXED; really the lane's rec_cap), `rep` list positions
// before kErrRecCap (really rec_cap + kRepSlack) --, so that a small batch reaches both ends.  A value only ever lowers its capacity
// (the buffers stay as large as they are); 0 or an empty field keeps it.  Never below kListCapFloor: a wave of kr_dedup_kernel that is
// over capacity goes on writing at position 0, kRepChunkMax entries at most, and the lowered list has that room too (a workgroup of
// kr_dedup_direct_kernel writes up to 4,096 there: inside the buffers, which hold kRepSlack positions and more whatever the knob says).
constexpr uint32_t kListCapFloor = kRepChunkMax;
struct ListCaps {
  uint64_t dist = 0, rep = 0;
  uint32_t lower(uint32_t cap, uint64_t to) const { return to ? (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>(to, kListCapFloor)) : cap; }
};
ListCaps debug_list_caps()
{
  ListCaps c;
  if (const char* e = getenv("KR_DEBUG_LIST_CAPS")) {
    char* end = nullptr;
    c.dist = strtoull(e, &end, 10);
    if (end && *end == ',') c.rep = strtoull(end + 1, nullptr, 10);
  }
  return c;
}

int check_errflags(uint32_t e)
{
  if (e & kErrRecCap) return kr::fail(KR_ERR_CAPACITY, "record buffer overflow: submit fewer reads per batch");
  if (e & kErrStack) return kr::fail(KR_ERR_CAPACITY, "colour work stack overflow (a colour expands into more pending work than the LDS stack and its spill hold)");
  if (e & kErrTable) return kr::fail(KR_ERR_CAPACITY, "global accumulator table overflow");
  if (e & kErrHitCap) return kr::fail(KR_ERR_CAPACITY, "hit tap buffer overflow");
  if (e & kErrItemCap) return kr::fail(KR_ERR_CAPACITY, "hit list overflow (more than 256 table hits per read on average): submit fewer reads per batch");
  return KR_OK;
}

// The device's view of the batch's per-read results: the arrays of `o` (the stream's, or a lane's), or for a tiled batch the real
// reads' (kr_tile_gather_kernel), their row ranges included
BatchOut result_out(const kr_stream* s, BatchOut o)
{
  if (s->batch.tiled) {
    const kr_stream::Tiles& t = s->tiles;
    o.rd_off = t.d_real_off.get(), o.rd_cnt = t.d_real_cnt.get(), o.rd_onmers = t.d_real_onmers.get(), o.rd_filt = t.d_real_filt.get(), o.rd_na = t.d_real_na.get();
    o.rd_roff = t.d_real_roff.get(), o.rd_rcnt = t.d_real_rcnt.get();
  }
  return o;
}

// Does this host batch hold long sequences, and does its tiled form fit the stream?  Then the batch in flight is tiled
// (Batch::tiled, nv, nlong).  Fills the tiled batch (bases with the
// k - 1 overlaps, offsets, tile flags, first tile of every real read, list of long sequences) into the pinned buffers.
int build_tiles(kr_stream* s, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads)
{
  const uint32_t k = s->ix->dix.k;
  // a long sequence of nt tiles takes nt - 1 reads more than the batch has: as many sequences as the stream has reads for
  // are tiled (in order), the others stay one wave's work each
  uint64_t spare = s->max_reads - nreads, nv = 0, nb = 0;
  uint32_t nlong = 0;
  std::vector<uint8_t>& tile_it = s->tile_choice;
  tile_it.assign(nreads, 0);
  for (uint32_t r = 0; r < nreads; ++r) {
    const uint64_t len = offsets[r + 1] - offsets[r];
    const TileShape sh = tile_shape(len, k);
    if (sh.nkm > s->tile_min_pos && sh.nt - 1 <= spare) {
      spare -= sh.nt - 1;
      tile_it[r] = 1;
      nv += sh.nt, nb += sh.bytes, ++nlong;
    } else {
      nv += 1, nb += len;
    }
  }
  if (nlong == 0) return KR_OK; // nothing to tile (or no room for a single sequence's tiles)
  kr_stream::Tiles& t = s->tiles;
  HIP_TRY(hipSetDevice(s->device));
  { // the per-read arrays, made by the first tiled batch.  A group that cannot be had is left empty (the submit reports the error, the
    // stream stays usable) and the next tiled batch asks again
    const uint64_t c = s->max_reads;
    if (!reserve_all(c + 1, t.h_voff, t.d_voff) ||
        !reserve_all(c, t.h_vtile, t.h_rfirst, t.d_vtile, t.d_rfirst, t.d_real_off, t.d_real_cnt, t.d_real_onmers, t.d_real_na, t.d_real_roff, t.d_real_rcnt) ||
        !reserve_all(2 * c, t.h_longs, t.d_longs, t.d_tile_filt, t.d_real_filt))
      return alloc_failed("build_tiles");
  }
  if (nb + 256 > t.h_bases.size() && !reserve_all(nb + nb / 4 + 256, t.h_bases, t.d_bases)) return alloc_failed("build_tiles");
  uint8_t* const h_bases = t.h_bases.get();
  uint64_t* const h_voff = t.h_voff.get();
  uint8_t* const h_vtile = t.h_vtile.get();
  uint32_t *const h_rfirst = t.h_rfirst.get(), *const h_longs = t.h_longs.get();
  uint64_t v = 0, pos = 0;
  uint32_t li = 0;
  for (uint32_t r = 0; r < nreads; ++r) {
    const uint8_t* src = bases + offsets[r];
    const uint64_t len = offsets[r + 1] - offsets[r];
    h_rfirst[r] = (uint32_t)v;
    if (tile_it[r]) {
      const uint64_t nt = tile_shape(len, k).nt;
      h_longs[2 * li] = (uint32_t)v, h_longs[2 * li + 1] = (uint32_t)nt, ++li;
      for (uint64_t ti = 0; ti < nt; ++ti) { // tile ti: k-mer positions [ti * kSegPos, ...), bases from the first one's start
        const uint64_t b0 = ti * kSegPos, b1 = std::min<uint64_t>(len, b0 + kSegPos + k - 1);
        memcpy(h_bases + pos, src + b0, b1 - b0);
        h_voff[v] = pos, h_vtile[v] = 1, ++v;
        pos += b1 - b0;
      }
    } else {
      memcpy(h_bases + pos, src, len);
      h_voff[v] = pos, h_vtile[v] = 0, ++v;
      pos += len;
    }
  }
  h_voff[v] = pos;
  s->batch.nv = (uint32_t)v, s->batch.nlong = nlong, s->batch.tiled = true;
  return KR_OK;
}

// The same for a batch whose bases and offsets are in HBM (KR_TILE_DEVICE): the kr_tile_lay_* kernels fill the device arrays on
// lane 0's stream, and the call waits for their summary {nv, nlong, bases} -- the tiled bases need room before they are copied, and
// a batch without a long sequence is submitted as it is.  Sequences are chosen by a prefix rule (kr_dev_tiles.inc).
int build_tiles_device(kr_stream* s, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads)
{
  kr_stream::Tiles& t = s->tiles;
  HIP_TRY(hipSetDevice(s->device));
  const uint64_t c = s->max_reads;
  const uint32_t nblk = (uint32_t)(((uint64_t)nreads + kTileBlock - 1) / kTileBlock);
  const uint64_t blk_cap = c / kTileBlock + 2;
  if (!reserve_all(c + 1, t.d_voff) ||
      !reserve_all(c, t.d_vtile, t.d_rfirst, t.d_real_off, t.d_real_cnt, t.d_real_onmers, t.d_real_na, t.d_real_roff, t.d_real_rcnt, t.d_choice, t.d_lread, t.d_vsrc) ||
      !reserve_all(2 * c, t.d_longs, t.d_tile_filt, t.d_real_filt) || !reserve_all(4 * blk_cap, t.d_bsum) || !reserve_all(4, t.d_sum, t.h_sum))
    return alloc_failed("build_tiles_device");
  hipStream_t st = s->lanes[0].stream;
  TileLayIO io;
  io.bases = bases, io.offsets = offsets;
  io.nreads = nreads, io.k = s->ix->dix.k, io.tile_min_pos = s->tile_min_pos;
  io.spare = s->max_reads - nreads;
  io.nblk = nblk;
  io.bsum_e = t.d_bsum.get(), io.bsum_v = io.bsum_e + blk_cap, io.bsum_b = io.bsum_v + blk_cap, io.bsum_l = io.bsum_b + blk_cap;
  io.choice = t.d_choice.get(), io.lread = t.d_lread.get(), io.vsrc = t.d_vsrc.get();
  io.voff = t.d_voff.get(), io.vtile = t.d_vtile.get(), io.rfirst = t.d_rfirst.get(), io.longs = t.d_longs.get();
  io.sum = t.d_sum.get();
  io.dst = nullptr;
  const dim3 bgrid(std::min<uint32_t>(nblk, 4096u));
  hipLaunchKernelGGL(kr_tile_lay_count_kernel, bgrid, dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_tile_lay_escan_kernel, dim3(1), dim3(1024), 0, st, io);
  hipLaunchKernelGGL(kr_tile_lay_choose_kernel, bgrid, dim3(256), 0, st, io);
  hipLaunchKernelGGL(kr_tile_lay_lscan_kernel, dim3(1), dim3(1024), 0, st, io);
  hipLaunchKernelGGL(kr_tile_lay_reads_kernel, bgrid, dim3(256), 0, st, io);
  // (a wave per long sequence, and there are at most `spare` + 1 ... nreads of them: the grid is bounded, the loop strides)
  hipLaunchKernelGGL(kr_tile_lay_tiles_kernel, dim3(std::min<uint32_t>((nreads + 3) / 4, 8192u)), dim3(256), 0, st, io);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(t.h_sum.get(), t.d_sum.get(), 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const uint64_t nv = t.h_sum.get()[0], nlong = t.h_sum.get()[1], nb = t.h_sum.get()[2];
  if (nlong == 0) return KR_OK; // nothing to tile (or no room for the first long sequence's tiles)
  if (nv > s->max_reads) return kr::fail(KR_ERR_ARG, "kr_batch_submit: the device offsets do not ascend"); // (the prefix rule keeps nv <= max_reads)
  if (nb + 256 > t.d_bases.size() && !t.d_bases.reserve(nb + nb / 4 + 256)) {
    t.h_bases.reset(); // (one capacity with d_bases: build_tiles asks for both again)
    return alloc_failed("build_tiles_device");
  }
  io.dst = t.d_bases.get();
  hipLaunchKernelGGL(kr_tile_lay_copy_kernel, dim3((uint32_t)std::min<uint64_t>((nv + 3) / 4, 16384u)), dim3(256), 0, st, io);
  HIP_TRY(hipGetLastError());
  s->batch.nv = (uint32_t)nv, s->batch.nlong = (uint32_t)nlong, s->batch.tiled = s->batch.tiles_on_device = true;
  return KR_OK;
}

// Runtime flags as template arguments: with_bools(f, b0, b1, ...) calls the generic lambda f with std::bool_constant<b0>{},
// std::bool_constant<b1>{}, ... so that a kernel family has ONE launch expression whatever its instantiation.
template <typename F>
void with_bools(F&& f)
{
  f();
}
template <typename F, typename... Bs>
void with_bools(F&& f, bool b, Bs... rest)
{
  auto bind = [&](auto c) { with_bools([&](auto... cs) { f(c, cs...); }, rest...); };
  b ? bind(std::true_type{}) : bind(std::false_type{});
}
template <int V>
using int_c = std::integral_constant<int, V>;
// The scan's lane-group shape as f(LG, CP, SLOTTED): 2^LG lanes x CP 16-byte chunks per probe.  Slotted tables by slot format; by
// log_g the packed ones (an index without a slotted copy, or format 9 when its filter slots are not used)
template <typename F>
void with_scan_shape(uint32_t slot_log2w, uint32_t log_g, F&& f)
{
  switch (slot_log2w) {
    case 5: return f(int_c<2>{}, int_c<2>{}, std::true_type{}); // 128-byte slots: 4 lanes x 2 chunks
    case 6: return f(int_c<2>{}, int_c<4>{}, std::true_type{}); // 256-byte slots: 4 lanes x 4 chunks
    case 7: return f(int_c<3>{}, int_c<4>{}, std::true_type{}); // 512-byte slots: 8 lanes x 4 chunks
    case 8: return f(int_c<2>{}, int_c<3>{}, std::true_type{}); // 192-byte slots: 4 lanes x 3 chunks
  }
  switch (log_g) {
    case 0: return f(int_c<0>{}, int_c<2>{}, std::false_type{});  // sparse tables: a lane per probe
    case 2: return f(int_c<2>{}, int_c<3>{}, std::false_type{});  // 4 lanes x 3 chunks = 48 entries per pass
    default: return f(int_c<3>{}, int_c<3>{}, std::false_type{}); // 8 lanes x 3 chunks = 96 entries per pass
  }
}

TileBatch tile_batch(const kr_stream* s)
{
  const kr_stream::Tiles& tl = s->tiles;
  const Batch& b = s->batch;
  return TileBatch{tl.d_vtile.get(), tl.d_longs.get(), tl.d_rfirst.get(), tl.d_tile_filt.get(), b.nv, b.nlong, b.nreads,
                   tl.d_real_off.get(), tl.d_real_cnt.get(), tl.d_real_onmers.get(), tl.d_real_filt.get(), tl.d_real_na.get(),
                   b.rows_mode ? tl.d_real_roff.get() : nullptr, b.rows_mode ? tl.d_real_rcnt.get() : nullptr};
}

// The stages of a lane's batch, each queued on the lane's stream (everything a stage needs is in L.in / L.out); launch_lane calls
// them in this order.
void launch_scan(kr_stream* s, Lane& L, bool single, bool tap)
{
  hipStream_t st = L.stream;
  const DevIndex& dix = s->ix->dix;
  BatchOut& o = L.out;
  const dim3 block(kScanWaves * kWave);
  auto grid = [&](uint32_t blocks) { return dim3(std::min<uint32_t>((L.nreads + kScanWaves - 1) / kScanWaves, blocks)); };
  // slotted tables: the scan as a software pipeline across probe groups (kr_dev_scan_pipe.inc); KR_SCAN_PIPE=0 (read when the
  // stream is made): the one-group-at-a-time kernel
  const bool pipe = s->scan_pipe;
  with_bools([&](auto SL, auto TAP) {
    if (s->fk) { // filter slots: one line per probe, candidates verified by the accumulate kernel
      hipLaunchKernelGGL((kr_scan_filt_kernel_t<KR_SCAN_FILT_DEPTH, KR_SCAN_FILT_WPE, SL.value, TAP.value>), grid(s->scan_filt_blocks), block, 0, st, dix, s->dp, L.in, o);
      return;
    }
    with_scan_shape(s->ix->slot_log2w, s->ix->log_g, [&](auto LG, auto CP, auto SLOTTED) {
      if constexpr (SLOTTED.value)
        if (pipe) {
          hipLaunchKernelGGL((kr_scan_pipe_kernel_t<LG.value, CP.value, KR_SCAN_DEPTH, KR_SCAN_PIPE_WPE, SL.value, TAP.value>), grid(s->scan_pipe_blocks), block, 0, st, dix, s->dp, L.in, o);
          return;
        }
      hipLaunchKernelGGL((kr_scan_kernel_t<LG.value, CP.value, SL.value, TAP.value, SLOTTED.value>), grid(s->scan_blocks), block, 0, st, dix, s->dp, L.in, o);
    });
  }, single, tap);
}

void launch_accumulate(kr_stream* s, Lane& L, bool single)
{
  hipStream_t st = L.stream;
  const DevIndex& dix = s->ix->dix;
  BatchOut& o = L.out;
  const uint32_t nreads = L.nreads;
  const Batch& b = s->batch;
  const TileBatch tb = tile_batch(s);
  if (b.tiled) // the tiles' hdist_filt moved aside: their keys are judged by the sequence's, in kr_tile_merge_kernel
    hipLaunchKernelGGL(kr_tile_filt_kernel, dim3(std::min<uint32_t>((b.nv + 255) / 256, 4096u)), dim3(256), 0, st, o, tb);
  const uint32_t lds = probe_lds_bytes(s->dp.np, o.bm_words), lds_lean = probe_lds_bytes(s->dp.np, o.bm_words, true);
  const uint32_t lds_lean2 = probe_lds_bytes(s->dp.np, o.bm_words, true, 2);
  static const bool no_lean2 = getenv("KR_DEBUG_NO_LEAN2") != nullptr; // (experiments: two-segment reads through the merge instantiation, as before round 3)
  const uint32_t grid_lean2 = (lds_lean2 <= 65536u && !no_lean2) ? std::min(nreads, s->nwaves_lean2) : 0u; // (very large trees: the two-segment layout does not fit a workgroup's LDS)
  const uint32_t grid_lean = std::min(nreads, s->nwaves_lean), grid_full = std::min(nreads, s->nwaves_full);
  const bool np5 = s->dp.np == 5 && !getenv("KR_DEBUG_NP0");
  with_bools([&](auto SL, auto NP5, auto FK) { // one-segment reads, two-segment reads, then the rest (merge instantiation)
    constexpr int NPV = NP5.value ? 5 : 0;
    hipLaunchKernelGGL((kr_acc_kernel_t<SL.value, NPV, false, 7, FK.value>), dim3(grid_lean), dim3(kWave), lds_lean, st, dix, s->dp, L.in, o);
    if (grid_lean2)
      hipLaunchKernelGGL((kr_acc_kernel_t<SL.value, NPV, false, 8, FK.value>), dim3(grid_lean2), dim3(kWave), lds_lean2, st, dix, s->dp, L.in, o);
    hipLaunchKernelGGL((kr_acc_kernel_t<SL.value, NPV, true, 7, FK.value>), dim3(grid_full), dim3(kWave), lds, st, dix, s->dp, L.in, o);
  }, single, np5, s->fk);
  if (b.tiled) { // the tiles' histograms added per key, the sequence's records at its first tile
    const uint32_t W = std::min<uint32_t>(32u, s->nwaves / std::max<uint32_t>(1u, b.nlong)); // adding waves per sequence
    if (W >= 2 && b.nlong <= s->nwaves) { // few long sequences: the adding spread over W waves each, then a wave per sequence emits
      hipLaunchKernelGGL(kr_tile_add_kernel, dim3(b.nlong * W), dim3(kWave), 0, st, dix, s->dp, o, tb, W);
      hipLaunchKernelGGL(kr_tile_merge_kernel<true>, dim3(b.nlong), dim3(kWave), (o.bm_words * 4u + 15u) & ~15u, st, dix, s->dp, o, tb);
    } else { // many: a wave per sequence does both
      hipLaunchKernelGGL(kr_tile_merge_kernel<false>, dim3(std::min<uint32_t>(b.nlong, s->nwaves)), dim3(kWave), (o.bm_words * 4u + 15u) & ~15u, st,
                         dix, s->dp, o, tb);
    }
  }
}

void launch_likelihood(kr_stream* s, Lane& L)
{ // the batch's distinct likelihood problems (de-duplication), then their minimisations
  hipStream_t st = L.stream;
  const DevIndex& dix = s->ix->dix;
  BatchOut& o = L.out;
  const bool np5 = s->llh.th == 4, direct = np5 && o.dd_nodes; // (the direct-mapped part: five planes only)
  const uint32_t places = kDdOslots * kDdClasses * o.dd_nodes;
  hipLaunchKernelGGL(kr_dedup_clear_kernel, dim3(4096), dim3(256), 0, st, o);
  if (o.dd_nodes) hipLaunchKernelGGL(kr_dedup_oslot_kernel, dim3(std::min<uint32_t>((L.nreads + kDdOslotReads - 1u) / kDdOslotReads, 1024u)), dim3(256), 0, st, o, L.nreads);
  hipLaunchKernelGGL(kr_dedup_kernel, dim3(kDedupBlocks), dim3(256), 0, st, o);
  if (direct) hipLaunchKernelGGL(kr_dedup_direct_kernel, dim3(std::min<uint32_t>((places + 4095u) / 4096u, 4096u)), dim3(256), 0, st, o);
  with_bools([&](auto NP5) {
    constexpr int NPV = NP5.value ? 5 : 0;
    hipLaunchKernelGGL(kr_llh_pre_kernel<NPV>, dim3(4096), dim3(256), 0, st, s->llh, dix, o);
    hipLaunchKernelGGL(kr_llh_kernel<NPV>, dim3(2048), dim3(256), 0, st, s->llh, dix, o);
  }, np5);
  if (direct) hipLaunchKernelGGL(kr_dedup_dv_kernel, dim3(std::min<uint32_t>((places + 1023u) / 1024u, 4096u)), dim3(256), 0, st, o);
}

// without --filter: a lane per read (kr_select_lane_kernel) by default; KR_SELECT_LANE=0 (read once per process): the wave-per-read kernel
// for every read
bool select_lane_default()
{
  static const bool lane_sel = !getenv("KR_SELECT_LANE") || atoi(getenv("KR_SELECT_LANE")) != 0;
  return lane_sel;
}
void launch_select(kr_stream* s, Lane& L, bool lane_sel = select_lane_default())
{
  hipStream_t st = L.stream;
  const DevIndex& dix = s->ix->dix;
  BatchOut& o = L.out;
  const uint32_t nreads = L.nreads;
  const uint32_t sgrid = std::min<uint32_t>((nreads + 7) / 8, 16384u);
  const bool filt = !s->dp.no_filter && s->dp.multi;
  const uint32_t lgrid = std::min<uint32_t>((nreads + 255) / 256, 8192u);
  with_bools([&](auto NP5, auto FILT) {
    constexpr int NPV = NP5.value ? 5 : 0;
    if (!FILT.value && lane_sel)
      hipLaunchKernelGGL((kr_select_lane_kernel<NPV>), dim3(lgrid), dim3(256), 0, st, s->llh, dix, s->dp, o, nreads);
    else
      hipLaunchKernelGGL((kr_select_kernel<NPV, FILT.value>), dim3(sgrid), dim3(256), 0, st, s->llh, dix, s->dp, o, nreads);
  }, s->llh.th == 4, filt);
}

// The output rows of a rows-mode batch, compact: (key, DIST) of the selected records, a read's rows contiguous.  Over the reads of
// the batch as the device has it: a tiled batch's rows come out in tiled-batch order, which is the caller's read order (a long
// sequence's rows lie at its first tile, its other tiles have none)
void launch_rows(kr_stream* s, Lane& L)
{
  hipStream_t st = L.stream;
  BatchOut& o = L.out;
  const uint32_t nreads = L.nreads, nblk = (nreads + kRowBlock - 1) / kRowBlock;
  hipLaunchKernelGGL(kr_rows_bsum_kernel, dim3(std::min<uint32_t>(nblk, 4096u)), dim3(256), 0, st, o, nreads);
  hipLaunchKernelGGL(kr_rows_bscan_kernel, dim3(1), dim3(1024), 0, st, o, nreads);
  with_bools([&](auto INDEXED) { hipLaunchKernelGGL(kr_rows_write_kernel<INDEXED.value>, dim3(std::min<uint32_t>(nblk, 8192u)), dim3(256), 0, st, o, nreads); },
             o.rows_indexed != 0);
  if (o.rows_indexed) hipLaunchKernelGGL(kr_rows_dlist_kernel, dim3(2048), dim3(256), 0, st, o);
}

// ... and as text (kr_dev_text.inc): lengths, block offsets, bytes.  Over the CALLER's reads -- ids are theirs --, so a tiled batch
// hands the kernels the real reads' row ranges (kr_tile_gather_kernel has run) and the caller's read count: the blocks here are
// blocks of the caller's reads, those of launch_rows blocks of the tiled batch's
int launch_text(kr_stream* s, Lane& L)
{
  hipStream_t st = L.stream;
  BatchOut o = L.out;
  uint32_t nreads = L.nreads;
  if (s->batch.tiled) {
    const kr_stream::Tiles& tl = s->tiles;
    o.rd_roff = tl.d_real_roff.get(), o.rd_rcnt = tl.d_real_rcnt.get(), o.rd_na = tl.d_real_na.get();
    nreads = s->batch.nreads;
  }
  const uint32_t nblk = (nreads + kRowBlock - 1) / kRowBlock;
  kr_stream::Text& tx = s->text;
  TextIO t{tx.d_ids, tx.d_id_off, s->batch.from.id_sep, s->ix->d_names.get(), s->ix->d_name_off.get(), tx.d_tlen, tx.d_bsum, tx.d_text, tx.text_cap, tx.d_total};
  HIP_TRY(hipMemsetAsync(tx.d_total, 0, 16, st));
  hipLaunchKernelGGL(kr_text_len_kernel, dim3(std::min<uint32_t>(nblk, 8192u)), dim3(256), 0, st, o, t, nreads);
  hipLaunchKernelGGL(kr_text_bscan_kernel, dim3(1), dim3(1024), 0, st, t.t_bsum, nblk, t.text_cap, t.total);
  hipLaunchKernelGGL(kr_text_write_kernel, dim3(std::min<uint32_t>(nblk, 8192u)), dim3(256), 0, st, o, t, nreads);
  HIP_TRY(hipMemcpyAsync(tx.h_total, tx.d_total, 16, hipMemcpyDeviceToHost, st));
  s->batch.text_made = true;
  return KR_OK;
}

void launch_gather(kr_stream* s, Lane& L)
{ // (tiled batches) per-read results of the real reads, for the views, the copies back, the text kernels and `place`
  hipLaunchKernelGGL(kr_tile_gather_kernel, dim3(std::min<uint32_t>((s->batch.nreads + 255) / 256, 4096u)), dim3(256), 0, L.stream, L.out, tile_batch(s));
}

void launch_rebase(kr_stream* s, Lane& L)
{
  hipStream_t st = L.stream;
  BatchOut& o = L.out;
  if (L.rec_base) // the result view indexes the stream's arrays, the lane's kernels its slice
    hipLaunchKernelGGL(kr_rebase_kernel, dim3(std::min<uint32_t>((L.nreads + 255) / 256, 1024u)), dim3(256), 0, st, o.rd_off, o.rd_cnt, L.nreads, L.rec_base);
}

// The batch in flight runs in P lanes: how it leaves the device (Batch::rows_mode / rows_indexed)
void set_lanes_and_row_modes(kr_stream* s, uint32_t P)
{
  Batch& b = s->batch;
  const uint32_t flags = b.flags;
  b.nlanes = P;
  // (a tiled batch keeps its record slots unless the caller asks for rows with KR_TILE_ROWS)
  b.rows_mode = (flags & KR_ROWS_ONLY) && !(flags & (KR_TAP_ACCS | KR_TAP_HITS)) && (!b.tiled || (flags & KR_TILE_ROWS)) && !getenv("KR_NO_ROW_COMPACTION");
  // KR_ROWS_INDEXED: 8-byte rows (key, position of DIST in the batch's distinct values).  One lane (a lane's positions are its own),
  // not tiled, no --filter (its select kernel writes rec_v, which the list of values aliases), no device text (its kernels read row_d)
  // (unindexed: this is the rerun of a batch whose list positions outgrew dist_list)
  b.rows_indexed = b.rows_mode && (flags & KR_ROWS_INDEXED) && P == 1 && !b.tiled && !(!s->dp.no_filter && s->dp.multi) && !b.has_ids() && !b.from.unindexed;
}
// Lane l's view of the output for a batch submitted with `flags` (set_lanes_and_row_modes has run): private scratch + slices of the stream's
// arrays, the lane's reads starting at r0.  One function for kr_batch_submit and kr_debug_select: the aliases of the row arrays
// (rec_rep / rep_dv, indexed: rec_d / rec_v) exist once.
void set_lane_view(kr_stream* s, Lane& L, uint32_t l, uint32_t r0, uint32_t flags, uint32_t lane_rec_cap, uint32_t lane_item_cap, uint32_t lane_item_room,
                   const ListCaps& list_caps)
{
  BatchOut& o = L.out;
  o = s->out;
  o.counters = L.d_counters, o.cursors = L.d_cursors;
  o.dd_table = L.d_dd, o.dd_slots = L.dd_slots;
  o.dd_direct = L.d_dd_direct, o.dd_dv = L.d_dd_dv, o.dd_ohist = L.d_dd_ohist, o.dd_oslot = L.d_dd_oslot;
  o.g_planes = L.d_g_planes, o.g_counts = L.d_g_counts, o.g_list = L.d_g_list, o.stk_spill = L.d_stk;
  o.rd_off += r0, o.rd_cnt += r0, o.rd_onmers += r0, o.rd_filt += 2ull * r0, o.rd_na += r0;
  o.rd_it_off += r0, o.rd_it_cnt += r0;
  o.long_list += r0 + 16ull * s->nwaves * l;
  o.items += (uint64_t)l * lane_item_cap, o.item_cap = lane_item_room;
  const uint64_t rb = L.rec_base;
  o.rec_read += rb, o.rec_key += rb, o.rec_hist += rb, o.rec_d += rb, o.rec_v += rb, o.rec_chisq += rb, o.rec_sel += rb;
  o.rec_w0 += rb, o.rec_rep += rb, o.rep_list += rb + (uint64_t)l * kRepSlack, o.rep_dv += rb + (uint64_t)l * kRepSlack;
  o.rec_cap = lane_rec_cap;
  o.rep_cap = list_caps.lower((uint32_t)std::min<uint64_t>((uint64_t)lane_rec_cap + kRepSlack, 0xFFFFFFFFull), list_caps.rep);
  o.dist_cap = list_caps.lower(lane_rec_cap, list_caps.dist);
  o.keep_v = ((flags & KR_ROWS_ONLY) && !(flags & KR_TAP_ACCS)) ? 0u : 1u;
  o.hist_always = (flags & KR_TAP_ACCS) ? 1u : 0u; // else a record's planes exist only where its packed word cannot describe it
  o.v_tile = s->batch.tiled ? s->tiles.d_vtile.get() : nullptr;
  o.rows_mode = s->batch.rows_mode ? 1u : 0u;
  o.rd_rcnt += r0, o.rd_roff += r0, o.row_bsum += r0 / kRowBlock + 2ull * l;
  o.row_key = o.rec_rep, o.row_d = reinterpret_cast<double*>(o.rep_dv); // (the lane's slices: dead once the select kernel has run)
  o.rows_indexed = s->batch.rows_indexed ? 1u : 0u;
  if (s->batch.rows_indexed) // (see BatchOut: the row kernel reads rec_rep here, so its output lies in rec_d; the values in rec_v)
    o.row_key = reinterpret_cast<uint32_t*>(o.rec_d), o.row_dix = o.row_key + lane_rec_cap, o.dist_list = o.rec_v;
}

// Queue the kernels of one lane on its stream.
int launch_lane(kr_stream* s, Lane& L, uint32_t flags)
{
  hipStream_t st = L.stream;
  BatchOut& o = L.out;
  { // about four chunks' worth of reads per wave, between 32 and kRecChunk slots (one shared counter serves ~90 M atomics/s:
    // a million-read batch must not take its slots 32 at a time)
    uint32_t per_wave = (uint32_t)std::min<uint64_t>(4ull * L.nreads / std::max<uint32_t>(1u, s->nwaves_lean), kRecChunk), c = 32;
    while (c < per_wave) c <<= 1;
    o.rec_chunk = std::min<uint32_t>(c, kRecChunk);
  }
  HIP_TRY(hipMemsetAsync(o.counters, 0, kCounterWords * 4, st));
  HIP_TRY(hipMemsetAsync(o.cursors, 0, kCurSets * kCursors * kCursorStride * 4, st));
  HIP_TRY(hipMemsetAsync(o.rec_key, 0, (uint64_t)o.rec_cap * 4, st));
  HIP_TRY(hipMemsetAsync(o.rec_sel, 0, (uint64_t)o.rec_cap, st));
  // the kernel chain of the index (see kr_index): wait for the previous batch's kernels, record behind ours
  const kr_index* ixp = s->ix;
  ChainLink chain(ixp, st);
  HIP_TRY(chain.opened);
  HIP_TRY(hipEventRecord(L.ev[kEvFirstKernel], st));
  const bool single = ixp->dix.nlibs == 1 && ixp->dix.m <= 64;
  launch_scan(s, L, single, (flags & KR_TAP_HITS) != 0);
  HIP_TRY(hipEventRecord(L.ev[kEvScanDone], st));
  HIP_TRY(hipEventRecord(L.ev[kEvAccStart], st));
  launch_accumulate(s, L, single);
  HIP_TRY(hipEventRecord(L.ev[kEvAccDone], st));
  HIP_TRY(hipEventRecord(L.ev[kEvLlhStart], st));
  launch_likelihood(s, L);
  launch_select(s, L);
  // (an untiled batch: rows, text, rebase as ever; a tiled one gathers the real reads' results between its rows and its text)
  if (o.rows_mode) launch_rows(s, L);
  if (s->batch.tiled) launch_gather(s, L);
  if (o.rows_mode && s->batch.has_ids())
    if (int rc = launch_text(s, L)) return rc;
  launch_rebase(s, L);
  HIP_TRY(hipEventRecord(L.ev[kEvLastKernel], st));
  HIP_TRY(chain.close(st));
  HIP_TRY(hipMemcpyAsync(L.h_counters, o.counters, kCounterWords * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipGetLastError());
  return KR_OK;
}

// ---- the steps every way into the stream shares ----

// Wait for the batch in flight: the staging buffers (bases, offsets, ids, the record finders' chunk) are about to be overwritten.
// The batch stays waitable and collectable as it was
int drain_batch(kr_stream* s)
{
  if (s->batch.submitted && !s->batch.waited)
    for (uint32_t l = 0; l < s->batch.nlanes; ++l) HIP_TRY(hipStreamSynchronize(s->lanes[l].stream));
  return KR_OK;
}

// A new batch begins here and nowhere else: a fresh record, then what its submit knows.  (`queued` is false for the crafted batch of
// kr_debug_select, which there is nothing to wait for.)  A batch that no record finder produced ends the last parse
Batch& begin_batch(kr_stream* s, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads, uint32_t flags, const BatchOrigin& from, bool queued = true)
{
  s->batch = Batch{};
  Batch& b = s->batch;
  b.submitted = queued;
  b.bases = bases, b.offsets = offsets, b.nreads = nreads, b.flags = flags, b.from = from;
  if (!from.parsed) s->parse = LastParse{};
  return b;
}

// A submit failed with `rc` (kr_last_error() says why) after work was queued on lanes 0 .. queued_lanes - 1: what was queued runs to
// its end (or fails with the same device error), nothing of this batch is handed out, and every later wait / collect on the stream
// reports this error until the next submit.  queued_lanes == 0: nothing is on the device yet, nothing is waited for
int fail_submit(kr_stream* s, int rc, uint32_t queued_lanes)
{
  const std::string msg = kr_last_error();
  for (uint32_t j = 0; j < queued_lanes; ++j)
    if (s->lanes[j].stream) (void)hipStreamSynchronize(s->lanes[j].stream);
  if (queued_lanes) (void)hipGetLastError();
  Batch& b = s->batch;
  b.nlanes = 0, b.nrecs = 0, b.nhits = 0;
  b.waited = true;
  b.rc = rc, b.msg = msg;
  return kr::fail(rc, msg);
}

// Reads [r0, r1) of a host batch on their way to the device, queued on `st`: the bases land at the same offsets in d_bases as in the
// caller's buffer (relative to offsets[0]), the offsets are rebased to the staging buffer and go to d_offsets + r0 + slot (every lane
// has its own r1 - r0 + 1 entries).  KR_BASES_PINNED: the caller's buffers are page-locked, the bases are copied from where they are
int stage_reads(kr_stream* s, hipStream_t st, const uint8_t* bases, const uint64_t* offsets, uint32_t r0, uint32_t r1, uint32_t slot, uint32_t flags)
{
  const uint64_t b0 = offsets[r0] - offsets[0], b1 = offsets[r1] - offsets[0];
  const uint64_t* ho = s->h_offsets; // [nreads + 1], shared boundary entries are written with the same value
  const uint8_t* src = bases + offsets[r0];
  if (!(flags & KR_BASES_PINNED)) {
    memcpy(s->h_bases + b0, src, b1 - b0);
    src = s->h_bases + b0;
  }
  if ((flags & KR_BASES_PINNED) && offsets[0] == 0)
    ho = offsets; // page-locked and already relative to the staging buffer: no host pass at all
  else
    for (uint32_t r = r0; r <= r1; ++r) s->h_offsets[r] = offsets[r] - offsets[0];
  HIP_TRY(hipMemcpyAsync(s->d_bases + b0, src, b1 - b0, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(s->d_offsets + r0 + slot, ho + r0, ((uint64_t)(r1 - r0) + 1) * 8, hipMemcpyHostToDevice, st));
  return KR_OK;
}

// The ids kr_batch_submit_text staged in page-locked memory, on their way to the device
int upload_ids(kr_stream* s, hipStream_t st)
{
  HIP_TRY(hipMemcpyAsync(s->text.d_ids, s->text.h_ids, s->batch.from.id_bytes, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(s->text.d_id_off, s->text.h_id_off, ((uint64_t)s->batch.nreads + 1) * 4, hipMemcpyHostToDevice, st));
  return KR_OK;
}

} // namespace

// kr_host_seek.inc: a batch submitted with KR_SEEK leaves the dist chain here
static int seek_check(const kr_stream* s, uint32_t flags, bool tile_ok, const char* who);
static int seek_submit(kr_stream* s, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads, uint32_t flags, const BatchOrigin& from);
static int seek_wait(kr_stream* s);

extern "C" {

int kr_stream_create(const kr_index* ix, const kr_params* p, uint32_t max_reads, uint64_t max_bases, uint64_t max_records,
                     kr_stream** out)
{
  kr::clear_error();
  if (!ix || !p || !out || max_reads == 0) return kr::fail(KR_ERR_ARG, "kr_stream_create: bad argument");
  if (p->hdist_th > KR_MAX_HDIST_TH) return kr::fail(KR_ERR_ARG, "--hdist-th above 16 is not supported (k-h <= 16 bounds hd)");
  HIP_TRY(hipSetDevice(ix->device));
  std::unique_ptr<kr_stream> s(new kr_stream());
  s->ix = ix;
  s->device = ix->device;
  s->params = *p;
  s->dp.th = p->hdist_th, s->dp.np = p->hdist_th + 1;
  s->dp.multi = p->multi, s->dp.no_filter = p->no_filter;
  s->dp.dmax_set = std::isnan(p->dist_max) ? 0 : 1;
  s->dp.dbg = getenv("KR_DEBUG_SKIP") ? (uint32_t)atoi(getenv("KR_DEBUG_SKIP")) : 0u;
  s->dp.chisq = p->chisq, s->dp.dist_max = p->dist_max;
  s->llh = make_llh_const(ix->dix.k, ix->dix.h, p->hdist_th);
  s->max_reads = max_reads, s->max_bases = max_bases;
  // lanes: host batches of at least 2 * lane_min_reads reads are cut into up to KR_LANES ranges (default 2: the copies of
  // one range overlap the kernels of the other; more ranges only add launches -- measured on the 10 GB index, reads
  // resident in HBM: 1 lane 13.3 ms per million reads, 2: 13.9, 4: 14.9, 8: 16.2, whatever share of the chip the
  // persistent scan / accumulate grids are given: the kernels of different lanes do not speed each other up)
  if (const char* e = getenv("KR_LANE_MIN_READS")) s->lane_min_reads = (uint32_t)std::max(1, atoi(e));
  if (const char* e = getenv("KR_TILE_MIN_POS")) s->tile_min_pos = (uint32_t)std::max<int>(kSegPos, atoi(e));
  s->lanes_for_device_input = getenv("KR_LANES_DEVICE") != nullptr; // experiments: lanes for batches already in HBM too
  {
    uint32_t want = getenv("KR_LANES") ? (uint32_t)std::max(1, atoi(getenv("KR_LANES"))) : 2u;
    s->max_lanes = std::max<uint32_t>(1u, std::min<uint32_t>(std::min<uint32_t>(want, kMaxLanes), max_reads / s->lane_min_reads));
  }
  const uint32_t ML = s->max_lanes;
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, ix->device));
  // resident waves per CU: LDS-limited (160 KiB per CU), VGPR-limited to 4 waves per SIMD
  const uint32_t nslots2 = std::max<uint32_t>(2u, 2u * ix->dix.nleaves), bm_words = ((nslots2 + 63) / 64) * 2;
  // resident accumulate waves per CU: LDS-limited, at most 16 by registers (4 per SIMD); reads are handed out
  // dynamically, so a grid that is not fully resident costs nothing
  if (probe_lds_bytes(p->hdist_th + 1, bm_words) > 65536u)
    return kr::fail(KR_ERR_ARG, "kr_stream_create: this many reference leaves with this --hdist-th needs more LDS than a workgroup has");
  uint32_t per_cu = std::min<uint32_t>(16u, 163840u / probe_lds_bytes(p->hdist_th + 1, bm_words));
  // the single-segment instantiation has a lean LDS layout and 96 registers: 5 waves per SIMD
  uint32_t per_cu_lean = std::min<uint32_t>(4u * KR_ACC_LEAN_WPE, 163840u / probe_lds_bytes(p->hdist_th + 1, bm_words, true));
  if (getenv("KR_DEBUG_ACC_WAVES")) {
    per_cu = std::min<uint32_t>(per_cu, (uint32_t)atoi(getenv("KR_DEBUG_ACC_WAVES")));
    per_cu_lean = std::min<uint32_t>(per_cu_lean, (uint32_t)atoi(getenv("KR_DEBUG_ACC_WAVES")));
  }
  uint32_t per_cu_lean2 = std::min<uint32_t>(16u, 163840u / probe_lds_bytes(p->hdist_th + 1, bm_words, true, 2)); // (4 waves per SIMD by registers)
  if (getenv("KR_DEBUG_ACC_WAVES")) per_cu_lean2 = std::min<uint32_t>(per_cu_lean2, (uint32_t)atoi(getenv("KR_DEBUG_ACC_WAVES")));
  s->nwaves_full = (uint32_t)prop.multiProcessorCount * std::max<uint32_t>(1u, per_cu);
  s->nwaves_lean = (uint32_t)prop.multiProcessorCount * std::max<uint32_t>(1u, per_cu_lean);
  s->nwaves_lean2 = std::min(s->nwaves_lean, (uint32_t)prop.multiProcessorCount * std::max<uint32_t>(1u, per_cu_lean2));
  const uint32_t np = s->dp.np;
  { // per-wave global scratch grows with the tree (100 B per leaf for the level-2 tables): bound the total by running
    // fewer waves on very large trees (reads are handed out dynamically, so any grid size is correct)
    const uint64_t np_ = np;
    const uint64_t tab_spill = std::min<uint32_t>(nslots2, 32768u), kt_spill = std::min<uint32_t>(nslots2, 65536u); // as below
    const uint64_t list_words = std::max<uint64_t>(nslots2, kEvSpill + tab_spill * ((np_ + 1) / 2 + 1) + kt_spill);
    const uint64_t per_wave = (uint64_t)nslots2 * np_ * (kPlaneWords + 1) * 4 + list_words * 4 + (uint64_t)kStackSpill * 8;
    // Round 6: the budget was 16 GB whatever the device had to spare, and on the 10,000-genome tree (2.7 MB of scratch a wave) it let
    // 3,000 accumulate waves of a lane run where the LDS admits 4,864: 3.1 waves per SIMD instead of 4.75, the kernel 32.7 ms per 8 M
    // reads instead of 25.6 (profiles/round6_syn10000_scratch_budget.txt).  Now: a sixth of the device memory that is free when the
    // stream is made, between 8 and 48 GB (KR_ACC_SCRATCH_GB overrides) -- 13 GB a lane is what full residency takes there.
    uint64_t budget_total = 16ull << 30;
    if (getenv("KR_ACC_SCRATCH_GB")) {
      budget_total = (uint64_t)std::max(1, atoi(getenv("KR_ACC_SCRATCH_GB"))) << 30;
    } else {
      size_t free_b = 0, total_b = 0;
      if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget_total = std::min<uint64_t>(48ull << 30, std::max<uint64_t>(8ull << 30, (uint64_t)free_b / 6));
    }
    const uint64_t budget = budget_total / ML;
    const uint32_t max_waves = (uint32_t)std::max<uint64_t>((uint64_t)prop.multiProcessorCount, budget / per_wave);
    s->nwaves_full = std::min(s->nwaves_full, max_waves);
    s->nwaves_lean = std::min(s->nwaves_lean, max_waves);
    s->nwaves_lean2 = std::min(s->nwaves_lean2, max_waves);
  }
  s->nwaves = std::max(s->nwaves_full, s->nwaves_lean);
  // default record capacity: up to 2 * leaves per read, at most 16 per read on average
  uint64_t per_read = std::min<uint64_t>(16, std::max<uint64_t>(8, (uint64_t)ix->dix.tree_nnodes + 1));
  uint64_t rc64 = max_records ? max_records : std::max<uint64_t>(1u << 16, (uint64_t)max_reads * per_read);
  s->rec_user_cap = rc64;
  // every resident wave of every lane may leave one partly used chunk behind: add that slack to the caller's bound
  s->rec_cap = (uint32_t)std::min<uint64_t>(rc64 + (uint64_t)ML * s->nwaves * kRecChunk, 1ull << 30);
  s->hit_cap = 1u << 22;
  int rc = 0;
  BatchOut& o = s->out;
  memset(&o, 0, sizeof(o));
#define SA(ptr, n) \
  if ((rc = salloc(s.get(), &ptr, (n)))) { kr_stream_destroy(s.release()); return rc; }
#define HA(ptr, n) \
  if ((rc = halloc(s.get(), &ptr, (n)))) { kr_stream_destroy(s.release()); return rc; }
#define HT(expr)                                                                                              \
  do { /* a failing HIP call: free what the stream holds so far (device and pinned allocations, events, streams) */ \
    hipError_t e__ = (expr);                                                                                  \
    if (e__ != hipSuccess) {                                                                                  \
      kr_stream_destroy(s.release());                                                                         \
      return kr::fail(e__ == hipErrorOutOfMemory ? KR_ERR_NOMEM : KR_ERR_NO_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    }                                                                                                         \
  } while (0)
  SA(s->d_bases, max_bases + 256);
  SA(s->d_offsets, (uint64_t)max_reads + ML);
  SA(o.rd_off, max_reads);
  SA(o.rd_cnt, max_reads);
  SA(o.rd_onmers, max_reads);
  SA(o.rd_filt, 2ull * max_reads);
  SA(o.rd_na, max_reads);
  SA(o.rec_read, s->rec_cap);
  SA(o.rec_key, s->rec_cap);
  SA(o.rec_hist, (uint64_t)s->rec_cap * np);
  SA(o.rec_d, s->rec_cap);
  SA(o.rec_v, s->rec_cap);
  SA(o.rec_chisq, s->rec_cap);
  SA(o.rec_sel, s->rec_cap);
  SA(o.rec_w0, s->rec_cap);
  SA(o.rec_rep, s->rec_cap);
  // (list positions are handed out in chunks of kRepChunk per wave of kr_dedup_kernel: room for every wave's unused tail behind
  //  a lane's records, so that a batch of all-distinct records cannot run past its slice)
  SA(o.rep_list, (uint64_t)s->rec_cap + (uint64_t)ML * kRepSlack);
  SA(o.rep_dv, (uint64_t)s->rec_cap + (uint64_t)ML * kRepSlack);
  o.dd_shift = getenv("KR_DD_SHIFT") ? (uint32_t)atoi(getenv("KR_DD_SHIFT")) : 1u; // measured: 1: 5.1 ms, 3: 5.6, 5: 6.9 (llh + select, syn1000)
  o.rec_cap = s->rec_cap;
  o.rec_stride = s->rec_cap;
  o.hit_cap = s->hit_cap;
  // item list between the two kernels: 256 hits per read on average, plus one partly used chunk per scan wave of every lane
  s->scan_blocks = (uint32_t)prop.multiProcessorCount * (4u * (ix->slot_log2w ? KR_SCAN_WPE_SLOT : KR_SCAN_WPE) / kScanWaves); // resident by construction (launch bounds)
  s->scan_pipe_blocks = (uint32_t)prop.multiProcessorCount * (4u * KR_SCAN_PIPE_WPE / kScanWaves);
  s->scan_filt_blocks = (uint32_t)prop.multiProcessorCount * (4u * KR_SCAN_FILT_WPE / kScanWaves);
  if (const char* e = getenv("KR_DEBUG_SCAN_BLOCKS_PER_CU"))
    s->scan_blocks = s->scan_pipe_blocks = s->scan_filt_blocks = (uint32_t)prop.multiProcessorCount * (uint32_t)std::max(1, atoi(e));
  s->fk = ix->slot_log2w == kSlotFilter && p->hdist_th <= kFiltMaxTh && !getenv("KR_NO_FILTER_SCAN");
  s->scan_pipe = !getenv("KR_SCAN_PIPE") || atoi(getenv("KR_SCAN_PIPE")) != 0;
  // KR_DEBUG_ITEM_CAP=n (tests): the scan of every lane is told that its item list holds n slots -- only ever fewer than it does
  if (const char* e = getenv("KR_DEBUG_ITEM_CAP")) s->item_cap_dbg = (uint32_t)std::min<uint64_t>(strtoull(e, nullptr, 10), 0xFFFFFFFFull);
  s->item_cap = (uint32_t)std::min<uint64_t>((uint64_t)max_reads * 256u + (uint64_t)ML * std::max(std::max(s->scan_blocks, s->scan_pipe_blocks), s->scan_filt_blocks) * kScanWaves * 2u * kItemChunk, 1ull << 31);
  if ((rc = new_item_list(s.get(), s->items))) { kr_stream_destroy(s.release()); return rc; }
  o.items = s->items.get();
  SA(o.rd_it_off, max_reads);
  SA(o.rd_it_cnt, max_reads);
  SA(o.long_list, (uint64_t)max_reads + 16ull * s->nwaves * ML);
  SA(o.rd_rcnt, max_reads);
  SA(o.rd_roff, max_reads);
  SA(o.row_bsum, (uint64_t)max_reads / kRowBlock + 2ull * ML + 2);
  o.nslots2 = nslots2;
  o.ev_spill = kEvSpill;
  o.tab_spill = std::min<uint32_t>(nslots2, 32768u); // (trees of up to 16,384 leaves: every passing key of a read fits, no read is set aside for the plane tables because of its records)
  o.kt_spill = std::min<uint32_t>(nslots2, 65536u);
  const uint32_t g_list_words = std::max<uint32_t>(nslots2, o.ev_spill + o.tab_spill * ((np + 1) / 2 + 1) + o.kt_spill /* table entries: up to (np + 1) / 2 words of 16-bit counters + the key */);
  o.g_list_words = g_list_words;
  o.bm_words = bm_words;
  // direct-mapped part of the likelihood de-duplication (kr_dev_likelihood.inc): th = 4 packs a record's problem in one word;
  // KR_DD_DIRECT=0 turns it off (A/B runs)
  const uint32_t dd_nodes = (s->llh.th == 4 && !(getenv("KR_DD_DIRECT") && atoi(getenv("KR_DD_DIRECT")) == 0)) ? ix->dix.tree_nnodes + 1u : 0u;
  o.dd_nodes = dd_nodes;
  if (dd_nodes) {
    std::vector<uint8_t> cls(1024, 0xFF); // histograms of 1 .. kDdMaxEvents events, five counts of at most 3, numbered in code order
    uint32_t ncls = 0;
    for (uint32_t code = 0; code < 1024; ++code) {
      uint32_t tot = 0;
      for (int x = 0; x < 5; ++x) tot += (code >> (2 * x)) & 3u;
      if (tot >= 1 && tot <= kDdMaxEvents) cls[code] = (uint8_t)ncls++;
    }
    if (ncls != kDdClasses) {
      kr_stream_destroy(s.release());
      return kr::fail(KR_ERR_ARG, "kr_stream_create: kDdClasses does not match kDdMaxEvents");
    }
    uint8_t* d_cls = nullptr;
    SA(d_cls, 1024);
    HT(hipMemcpy(d_cls, cls.data(), 1024, hipMemcpyHostToDevice));
    o.dd_cls = d_cls;
  }
  for (uint32_t l = 0; l < ML; ++l) {
    Lane& L = s->lanes[l];
    // HIP streams are a scarce resource (the runtime folds every stream after the third onto one hardware queue unless
    // GPU_MAX_HW_QUEUES says otherwise): lane 0 has one from the start, the others get theirs when a batch first uses them
    if (l == 0) HT(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    for (auto& e : L.ev) HT(hipEventCreate(&e));
    SA(L.d_counters, kCounterWords);
    SA(L.d_cursors, kCurSets * kCursors * kCursorStride);
    // lane 0 may be the only lane of a batch; a later lane never holds more than half of one
    const uint32_t lane_recs = l == 0 ? s->rec_cap : s->rec_cap / 2;
    L.dd_slots = std::min<uint32_t>(next_pow2(std::max<uint32_t>(2048u, lane_recs >> o.dd_shift)), 1u << 26);
    SA(L.d_dd, L.dd_slots);
    if (dd_nodes) {
      SA(L.d_dd_direct, ((uint64_t)kDdOslots * kDdClasses * dd_nodes + 3) & ~3ull);
      SA(L.d_dd_dv, ((uint64_t)kDdOslots * kDdClasses * dd_nodes + 3) & ~3ull);
      SA(L.d_dd_ohist, 260);
      SA(L.d_dd_oslot, 256);
    }
    SA(L.d_stk, (uint64_t)s->nwaves * kStackSpill);
    SA(L.d_g_planes, (uint64_t)s->nwaves * nslots2 * np * kPlaneWords);
    SA(L.d_g_counts, (uint64_t)s->nwaves * nslots2 * np);
    SA(L.d_g_list, (uint64_t)s->nwaves * g_list_words);
    // on the lane's own stream and waited for: it does not synchronise with the null stream, and a
    // multi-GB clear (large trees) would otherwise still be running when the first batch arrives
    HT(hipMemsetAsync(L.d_g_planes, 0, (uint64_t)s->nwaves * nslots2 * np * kPlaneWords * 4, s->lanes[0].stream));
    HT(hipMemsetAsync(L.d_g_counts, 0, (uint64_t)s->nwaves * nslots2 * np * 4, s->lanes[0].stream));
    HA(L.h_counters, kCounterWords);
  }
  HT(hipStreamSynchronize(s->lanes[0].stream));
  HA(s->h_bases, max_bases + 256);
  HA(s->h_offsets, (uint64_t)max_reads + 1);
  HA(s->h_rd_off, max_reads);
  HA(s->h_rd_cnt, max_reads);
  HA(s->h_rd_onmers, max_reads);
  HA(s->h_rd_filt, 2ull * max_reads);
  HA(s->h_rd_na, max_reads);
#undef SA
#undef HA
#undef HT
  *out = s.release();
  return KR_OK;
}

void kr_stream_destroy(kr_stream* s)
{
  if (!s) return;
  (void)hipSetDevice(s->device);
  for (auto& L : s->lanes)
    if (L.stream) (void)hipStreamSynchronize(L.stream);
  for (void* p : s->dallocs) (void)hipFree(p);
  for (void* p : s->hallocs) (void)hipHostFree(p);
  for (auto& L : s->lanes) {
    for (auto& e : L.ev)
      if (e) (void)hipEventDestroy(e);
    if (L.stream) (void)hipStreamDestroy(L.stream);
  }
  for (hipStream_t st : s->moved_streams) (void)hipStreamDestroy(st);
  if (s->fq.ev_parse0) (void)hipEventDestroy(s->fq.ev_parse0);
  if (s->fq.ev_parse1) (void)hipEventDestroy(s->fq.ev_parse1);
  if (s->bgzf.ev0) (void)hipEventDestroy(s->bgzf.ev0);
  if (s->bgzf.ev1) (void)hipEventDestroy(s->bgzf.ev1);
  if (s->bgzf_out.ev0) (void)hipEventDestroy(s->bgzf_out.ev0);
  if (s->bgzf_out.ev1) (void)hipEventDestroy(s->bgzf_out.ev1);
  for (auto& e : s->seek.ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : s->extract.ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : s->extract.ev_x)
    if (e) (void)hipEventDestroy(e);
  delete s; // (every DevBuf / PinBuf of the stream frees itself here: the device is set, the lanes' streams have been waited for)
}

static int submit_batch(kr_stream* s, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads, uint32_t flags, const BatchOrigin& from);
int kr_batch_submit(kr_stream* s, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads, uint32_t flags)
{
  return submit_batch(s, bases, offsets, nreads, flags, BatchOrigin{});
}

// ---- report text on the device (include/krepp_amd.h; kernels: kr_dev_text.inc) ----
static int text_buffers(kr_stream* s, uint64_t max_text_bytes, uint64_t max_id_bytes);
int kr_stream_text_enable(kr_stream* s, const kr_host_index* h, uint64_t max_text_bytes, uint64_t max_id_bytes)
{
  kr::clear_error();
  if (!s || !h || max_text_bytes == 0 || max_id_bytes == 0) return kr::fail(KR_ERR_ARG, "kr_stream_text_enable: bad argument");
  if (s->text.on && !s->text.seek_only) return kr::fail(KR_ERR_STATE, "kr_stream_text_enable: already enabled");
  if (s->text.on && (max_text_bytes > s->text.text_cap || max_id_bytes > s->text.id_cap))
    return kr::fail(KR_ERR_STATE, "kr_stream_text_enable: kr_stream_seek_enable made smaller text buffers on this stream: enable the dist text first");
  if (max_id_bytes >= (1ull << 32)) return kr::fail(KR_ERR_ARG, "kr_stream_text_enable: the ids of one batch must stay below 4 GB");
  HIP_TRY(hipSetDevice(s->ix->device));
  const kr_index* ix = s->ix;
  { // the node names, once per index
    std::lock_guard<std::mutex> lk(ix->chain_mu);
    if (!ix->d_names.get()) {
      const uint32_t nn = ix->dix.tree_nnodes;
      std::vector<uint32_t> off((size_t)nn + 2, 0);
      std::string blob;
      for (uint32_t se = 0; se <= nn; ++se) {
        off[se] = (uint32_t)blob.size();
        blob += kr_host_index_node_name(h, se);
      }
      off[(size_t)nn + 1] = (uint32_t)blob.size();
      DevBuf<char> dn; // (local until both are filled: an early return frees them)
      DevBuf<uint32_t> dofs;
      if (!dn.reserve(blob.size())) return alloc_failed("kr_stream_text_enable: node names");
      if (!dofs.reserve(off.size())) return kr::fail(KR_ERR_NOMEM, "kr_stream_text_enable: out of device memory");
      HIP_TRY(hipMemcpy(dn.get(), blob.data(), blob.size(), hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(dofs.get(), off.data(), off.size() * 4, hipMemcpyHostToDevice));
      ix->d_name_off.swap(dofs);
      ix->d_names.swap(dn); // (freed with the index)
    }
  }
  kr_stream::Text& t = s->text;
  if (t.on) { // (the seek text's buffers serve: the node names were all that was missing)
    t.seek_only = false;
    return KR_OK;
  }
  return text_buffers(s, max_text_bytes, max_id_bytes);
}

// the buffers of the device text, for kr_stream_text_enable and kr_stream_seek_enable
static int text_buffers(kr_stream* s, uint64_t max_text_bytes, uint64_t max_id_bytes)
{
  kr_stream::Text& t = s->text;
  int rc = 0;
  const uint64_t nblk = (uint64_t)s->max_reads / kRowBlock + 2;
  if ((rc = salloc(s, &t.d_ids, max_id_bytes)) || (rc = salloc(s, &t.d_id_off, (uint64_t)s->max_reads + 1)) || (rc = salloc(s, &t.d_tlen, (uint64_t)s->max_reads)) ||
      (rc = salloc(s, &t.d_bsum, nblk)) || (rc = salloc(s, &t.d_total, 2)) || (rc = salloc(s, &t.d_text, max_text_bytes)) ||
      (rc = halloc(s, &t.h_ids, max_id_bytes)) || (rc = halloc(s, &t.h_id_off, (uint64_t)s->max_reads + 1)) || (rc = halloc(s, &t.h_total, 2)))
    return rc;
  // (the page-locked buffer the text comes back into is made by the first batch that needs it, as large as that batch's text + 25 %:
  //  page-locking max_text_bytes up front -- 400 MB a worker of the CLI -- was 0.2-0.3 s of a run that takes half a second on an
  //  index of few references, where a batch's text is 15 MB; round 6)
  t.id_cap = max_id_bytes, t.text_cap = max_text_bytes;
  t.on = true;
  return KR_OK;
}

int kr_batch_submit_text(kr_stream* s, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads, uint32_t flags, const char* ids,
                         const uint32_t* id_off, uint32_t id_sep)
{
  kr::clear_error();
  if (!s || !ids || !id_off) return kr::fail(KR_ERR_ARG, "kr_batch_submit_text: null argument");
  if (!s->text.on) return kr::fail(KR_ERR_STATE, "kr_batch_submit_text: kr_stream_text_enable first");
  if (nreads == 0 || nreads > s->max_reads) return kr::fail(KR_ERR_ARG, "kr_batch_submit_text: nreads out of range for this stream");
  if (flags & KR_SEEK) {
    if (int rc = seek_check(s, flags, false, "kr_batch_submit_text")) return rc;
  } else if (s->text.seek_only) {
    return kr::fail(KR_ERR_STATE, "kr_batch_submit_text: this stream's text buffers are kr_stream_seek_enable's: kr_stream_text_enable for the dist text");
  }
  if (flags & (KR_TAP_ACCS | KR_TAP_HITS)) return kr::fail(KR_ERR_ARG, "kr_batch_submit_text: taps keep record slots, not rows");
  const uint64_t nb = (uint64_t)id_off[nreads] - id_off[0];
  if (nb > s->text.id_cap) return kr::fail(KR_ERR_CAPACITY, "kr_batch_submit_text: the batch's ids exceed max_id_bytes: submit fewer reads per batch");
  HIP_TRY(hipSetDevice(s->ix->device));
  if (int rc = drain_batch(s)) return rc; // the staging buffers belong to the batch in flight
  kr_stream::Text& t = s->text;
  memcpy(t.h_ids, ids + id_off[0], nb);
  for (uint32_t r = 0; r <= nreads; ++r) {
    if (r && id_off[r] < id_off[r - 1] + id_sep) return kr::fail(KR_ERR_ARG, "kr_batch_submit_text: id offsets must ascend by at least id_sep");
    t.h_id_off[r] = id_off[r] - id_off[0];
  }
  BatchOrigin from;
  from.ids = kIdsHost, from.id_bytes = nb, from.id_sep = id_sep;
  return submit_batch(s, bases, offsets, nreads, (flags & KR_SEEK) ? flags : flags | KR_ROWS_ONLY, from);
}

int kr_batch_collect_text(kr_stream* s, const char** text, uint64_t* len)
{
  kr::clear_error();
  if (!s || !text || !len) return kr::fail(KR_ERR_ARG, "kr_batch_collect_text: null argument");
  if (!s->batch.submitted || !s->batch.has_ids()) return kr::fail(KR_ERR_STATE, "kr_batch_collect_text: no batch submitted with kr_batch_submit_text");
  const int rc = kr_batch_wait(s);
  if (rc) return rc;
  kr_stream::Text& t = s->text;
  if (!s->batch.text_made) return kr::fail(KR_ERR_UNSUPPORTED, "kr_batch_collect_text: the batch left the device as record slots (long sequences; submit with KR_TILE_ROWS for device text): kr_batch_collect + kr_format_dist");
  if (t.h_total[1] & kTextOverCap) return kr::fail(KR_ERR_CAPACITY, "the batch's report text exceeds max_text_bytes: submit fewer reads per batch");
  if (t.h_total[1] & kTextBadNum) return kr::fail(KR_ERR_UNSUPPORTED, "kr_batch_collect_text: a DIST outside [0, 1000): kr_batch_collect + kr_format_dist");
  HIP_TRY(hipSetDevice(s->ix->device));
  const uint64_t n = t.h_total[0];
  if (n) {
    if (n > t.h_text.size() && !t.h_text.reserve(std::min<uint64_t>(t.text_cap, n + n / 4 + (1u << 20)))) return alloc_failed("kr_batch_collect_text");
    HIP_TRY(hipMemcpyAsync(t.h_text.get(), t.d_text, n, hipMemcpyDeviceToHost, s->lanes[0].stream));
    HIP_TRY(hipStreamSynchronize(s->lanes[0].stream));
  }
  *text = t.h_text.get() ? t.h_text.get() : "";
  *len = n;
  return KR_OK;
}

static int submit_batch(kr_stream* s, const uint8_t* bases, const uint64_t* offsets, uint32_t nreads, uint32_t flags, const BatchOrigin& from)
{
  kr::clear_error();
  if (!s || !bases || !offsets) return kr::fail(KR_ERR_ARG, "kr_batch_submit: null argument");
  if (nreads == 0 || nreads > s->max_reads) return kr::fail(KR_ERR_ARG, "kr_batch_submit: nreads out of range for this stream");
  // every argument is checked before the stream's state is touched: a rejected submit leaves the previous batch as it was
  if (!(flags & KR_BASES_DEVICE) && offsets[nreads] - offsets[0] > s->max_bases)
    return kr::fail(KR_ERR_ARG, "kr_batch_submit: more bases than the stream was created for");
  if (flags & KR_SEEK) {
    if (int rc = seek_check(s, flags, false, "kr_batch_submit")) return rc;
    return seek_submit(s, bases, offsets, nreads, flags, from);
  }
  HIP_TRY(hipSetDevice(s->ix->device));
  (void)hipGetLastError(); // a stale error of an earlier, unrelated call on this thread is not this batch's
  if (int rc = drain_batch(s)) return rc;
  Batch& b = begin_batch(s, bases, offsets, nreads, flags, from);
  // long sequences across waves: a host batch that holds any is submitted as a batch of tiles (kr_dev_tiles.inc); the hit tap
  // (tests) reports positions within reads and keeps the batch as it is
  const bool may_tile = !(flags & KR_TAP_HITS) && !from.untiled && !getenv("KR_NO_TILES");
  if (may_tile && !(flags & KR_BASES_DEVICE)) {
    if (int rc = build_tiles(s, bases, offsets, nreads)) return fail_submit(s, rc, 0);
  } else if (may_tile && (flags & KR_TILE_DEVICE)) { // ... and a batch in HBM whose caller asks for it: the same arrays, laid out by kernels on lane 0
    if (int rc = build_tiles_device(s, bases, offsets, nreads)) return fail_submit(s, rc, 1);
  }
  // lanes of this batch: ranges of at least lane_min_reads reads; the hit tap (tests) keeps one hit buffer, hence one lane
  uint32_t P = std::min<uint32_t>(s->max_lanes, std::max<uint32_t>(1u, nreads / s->lane_min_reads));
  if (flags & KR_TAP_HITS) P = 1;
  if (b.tiled) P = 1; // (a sequence's tiles belong to one launch)
  if ((flags & KR_BASES_DEVICE) && !s->lanes_for_device_input) P = 1; // nothing to copy, nothing to overlap
  if (b.has_ids()) P = 1; // (one text buffer, one prefix over the reads)
  set_lanes_and_row_modes(s, P);
  const ListCaps list_caps = debug_list_caps();
  if (flags & KR_TAP_HITS) {
    if (!reserve_all(s->hit_cap, s->d_hits, s->h_hits)) return alloc_failed("kr_batch_submit: hit tap buffers");
    s->out.hits = s->d_hits.get();
  }
  const uint32_t lane_rec_cap = P == 1 ? s->rec_cap : (s->rec_cap / P) & ~63u;
  const uint32_t lane_item_cap = s->item_cap / P; // (the lane's slice; what its scan may use of it: lane_item_room)
  const uint32_t lane_item_room = s->item_cap_dbg ? std::min(lane_item_cap, s->item_cap_dbg) : lane_item_cap;
  auto submit_lane = [&](uint32_t l) -> int {
    Lane& L = s->lanes[l];
    const uint32_t r0 = (uint32_t)((uint64_t)nreads * l / P), r1 = (uint32_t)((uint64_t)nreads * (l + 1) / P);
    L.read0 = r0, L.nreads = r1 - r0, L.rec_base = l * lane_rec_cap, L.rec_cap = lane_rec_cap, L.nrecs = 0;
    if (!L.stream) HIP_TRY(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
    hipStream_t st = L.stream;
    HIP_TRY(hipEventRecord(L.ev[kEvCopyIn], st));
    if (b.tiled) { // the tiled batch: its own bases and offsets, and what the tile kernels need
      kr_stream::Tiles& t = s->tiles;
      if (!b.tiles_on_device) { // (else the layout kernels wrote them, on this stream)
        HIP_TRY(hipMemcpyAsync(t.d_bases.get(), t.h_bases.get(), t.h_voff.get()[b.nv], hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t.d_voff.get(), t.h_voff.get(), ((uint64_t)b.nv + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t.d_vtile.get(), t.h_vtile.get(), b.nv, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t.d_rfirst.get(), t.h_rfirst.get(), (uint64_t)nreads * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(t.d_longs.get(), t.h_longs.get(), (uint64_t)b.nlong * 8, hipMemcpyHostToDevice, st));
      }
      L.in.bases = t.d_bases.get();
      L.in.offsets = t.d_voff.get();
      L.nreads = b.nv;
    } else if (flags & KR_BASES_DEVICE) {
      L.in.bases = bases;
      L.in.offsets = offsets + r0;
    } else {
      if (int rc = stage_reads(s, st, bases, offsets, r0, r1, l, flags)) return rc;
      L.in.bases = s->d_bases;
      L.in.offsets = s->d_offsets + r0 + l;
    }
    if (from.ids == kIdsHost && (!b.tiled || b.rows_mode)) // (a tiled batch that keeps its record slots has no text kernels to read them)
      if (int rc = upload_ids(s, st)) return rc;
    L.in.nreads = L.nreads;
    set_lane_view(s, L, l, r0, flags, lane_rec_cap, lane_item_cap, lane_item_room, list_caps);
    return launch_lane(s, L, flags);
  };
  for (uint32_t l = 0; l < P; ++l)
    if (int rc = submit_lane(l)) return fail_submit(s, rc, l + 1); // (lane l failed somewhere between its copies and its last launch)
  return KR_OK;
}

// How kr_batch_wait combines the lanes' counters into kr_stream::h_counters (CounterSlot, kr_dev_common.inc); a slot that is not
// listed is read per lane only and stays 0 there
enum CounterCombine { kSum, kMax, kOr };
struct CounterRule {
  CounterSlot slot;
  CounterCombine how;
};
constexpr CounterRule kCounterRules[] = {
  {kCtErr, kOr}, {kCtL2Reads, kSum}, {kCtTapHits, kSum}, {kCtRecords, kSum}, {kCtItemSlots, kSum},
  {kCtStEvents, kSum}, {kCtStKeys, kSum}, {kCtStBatches, kSum}, {kCtStBig, kSum}, {kCtStLevelTiles, kSum}, {kCtStMaxKeys, kMax}, {kCtStMaxEvents, kMax},
  {kCtCycLevel, kSum}, {kCtCycFinalize, kSum}, {kCtCycRead, kSum},
  {kCtProblems, kSum}, {kCtStackSpills, kSum}, {kCtTileHoles, kSum},
  {kCtFpEntered, kSum}, {kCtFpFalseEarly, kSum}, {kCtFpCompact, kSum}, {kCtFpFalseCompacted, kSum}, {kCtFpBigRead, kSum}, {kCtFpOneBatch, kSum},
  {kCtFpMultiBatch, kSum}, {kCtFpExtraBatches, kSum}, {kCtFpDupCalls, kSum}, {kCtFpDupMoved, kSum},
  {kCtGeEntered1, kSum}, {kCtGeEntered2, kSum}, {kCtGeEnteredMerge, kSum}, {kCtGeFused, kSum}, {kCtGeSparse, kSum}, {kCtGeBig, kSum},
  {kCtGeExtraBatches, kSum}, {kCtGeKeytabGlobal, kSum}, {kCtGeNoFit, kSum}, {kCtRdSetAside, kSum}, {kCtRdPlaneRedo, kSum},
};
static_assert(kCtPathCount == 21, "kr_debug_acc_paths: the slot names in krepp_amd/capi.py (ACC_PATHS) follow CounterSlot");

// After a large one-lane batch: how fast did the scan run on the item list in use?  Keep the faster of {the list set aside, the
// one in use}, and while trials are left put a freshly allocated one in use for the next batch.  KR_ITEM_PLACEMENT_TRIALS
// allocations per stream, DEFAULT kItemPlacementTrials since round 5 (0 before: the benchmark asked for five and the CLI got none,
// so a product process whose list had landed on a 46 ms piece of memory stayed at ~105 M reads/s where bench.py reported 113 M).
// Only a stream that is given batches of a million reads and more ever tries: a trial is a multi-GB hipMalloc / hipFree inside
// kr_batch_wait during the stream's first 3 + 2 x trials large batches (hipFree synchronises the device under every other stream),
// nothing afterwards; one spare list at a time, never the last of the device's memory (free >= 2 x the list), and never an error:
// a failed allocation ends the trials.  KR_ITEM_PLACEMENT_TRIALS=0 turns them off.
constexpr int kItemPlacementTrials = 5; // P(all six lists on the slow level) = 2 % where half of the allocations land there
int item_placement_step(kr_stream* s)
{
  kr_stream::ItemPlacement& ip = s->ipl;
  if (ip.trials_left < 0) {
    const char* e = getenv("KR_ITEM_PLACEMENT_TRIALS");
    ip.trials_left = (e && *e) ? std::max(0, atoi(e)) : kItemPlacementTrials;
  }
  if (ip.trials_left == 0 && !ip.aside.get()) return KR_OK;
  if (s->batch.tiled || s->batch.nreads < 1000000u || (s->batch.flags & KR_TAP_HITS)) return KR_OK; // (small batches: the launch is not what their time is)
  float ms = 0;
  for (uint32_t l = 0; l < s->batch.nlanes; ++l) { // (the lanes of a batch work in slices of the one list: their scan times are added)
    float ml = 0;
    if (hipEventElapsedTime(&ml, s->lanes[l].ev[kEvFirstKernel], s->lanes[l].ev[kEvScanDone]) != hipSuccess) {
      (void)hipGetLastError(); // (not this batch's business: leave no sticky error behind)
      return KR_OK;
    }
    ms += ml;
  }
  const double ns = (double)ms * 1e6 / s->batch.nreads;
  static const bool verbose = getenv("KR_ITEM_PLACEMENT_VERBOSE") != nullptr;
  if (ip.settling > 0) { // an early launch on this list (the stream's own, or a trial): a later one counts
    --ip.settling;
    if (verbose) fprintf(stderr, "[krepp_amd] item list: early launch %.3f ns per read (not measured)\n", ns);
    return KR_OK;
  }
  if (ip.aside.get()) { // the list in use was a trial
    const bool better = ns < ip.best_ns * 0.985;
    if (verbose) fprintf(stderr, "[krepp_amd] item list trial %u: %.3f ns per read against %.3f: %s\n", ip.tried, ns, ip.best_ns, better ? "kept" : "dropped");
    if (better) {
      ip.best_ns = ns, ++ip.kept_new;
    } else {
      s->items.swap(ip.aside);
      s->out.items = s->items.get();
    }
    ip.aside.reset(); // (the loser)
  } else {
    ip.best_ns = ns;
    if (verbose) fprintf(stderr, "[krepp_amd] item list as allocated: %.3f ns per read\n", ns);
  }
  if (ip.trials_left > 0) {
    --ip.trials_left;
    const uint64_t bytes = (uint64_t)s->item_cap * sizeof(uint2);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < 2 * bytes) { // never the last of the memory: somebody else may want it
      (void)hipGetLastError();
      ip.trials_left = 0;
      return KR_OK;
    }
    if (!ip.aside.renew(s->item_cap)) {
      (void)hipGetLastError();
      ip.trials_left = 0;
      return KR_OK;
    }
    s->items.swap(ip.aside); // the fresh list in use, the best so far aside
    s->out.items = s->items.get();
    ip.settling = 1;
    ++ip.tried;
  }
  return KR_OK;
}

// kr_batch_wait runs the batch it has just waited for again, from the batch's own record with one mode bit set: the same arguments,
// the same ids (a text batch stays one: staged ids are still staged, a record finder's still lie in HBM), the same origin
static int rerun_batch(kr_stream* s, bool BatchOrigin::*mode)
{
  const Batch was = s->batch; // (a copy: submit_batch begins a fresh record)
  BatchOrigin from = was.from;
  from.*mode = true;
  const int rc = submit_batch(s, was.bases, was.offsets, was.nreads, was.flags, from);
  return rc ? rc : kr_batch_wait(s);
}

int kr_batch_wait(kr_stream* s)
{
  if (!s || !s->batch.submitted) return kr::fail(KR_ERR_STATE, "kr_batch_wait: nothing submitted");
  if (s->batch.waited) return s->batch.rc ? kr::fail(s->batch.rc, s->batch.msg) : KR_OK;
  if (s->batch.seek) return seek_wait(s);
  HIP_TRY(hipSetDevice(s->ix->device));
  memset(s->h_counters, 0, sizeof(s->h_counters));
  uint32_t extent = 0;
  bool lane_full = false;
  for (uint32_t l = 0; l < s->batch.nlanes; ++l) {
    Lane& L = s->lanes[l];
    HIP_TRY(hipStreamSynchronize(L.stream)); // kernels done, counters in L.h_counters
    const uint32_t* c = L.h_counters;
    L.nrecs = std::min(c[kCtRecSlots], L.rec_cap);
    L.nrows = c[kCtRows];
    extent = std::max(extent, L.nrecs ? L.rec_base + L.nrecs : 0u);
    lane_full = lane_full || c[kCtRecSlots] > L.rec_cap;
    for (const CounterRule& r : kCounterRules) {
      uint32_t& a = s->h_counters[r.slot];
      a = r.how == kSum ? a + c[r.slot] : (r.how == kMax ? std::max(a, c[r.slot]) : (a | c[r.slot]));
    }
  }
  s->batch.waited = true;
  const uint32_t* hc = s->h_counters;
  if (s->dp.dbg & 512u)
    fprintf(stderr, "[kr stats] reads %u events %u keys %u batches %u big %u level-tiles %u max keys %u max events %u records %u distinct likelihood problems (list positions) %u\n", s->batch.nreads,
            hc[kCtStEvents], hc[kCtStKeys], hc[kCtStBatches], hc[kCtStBig], hc[kCtStLevelTiles], hc[kCtStMaxKeys], hc[kCtStMaxEvents], hc[kCtRecords], hc[kCtProblems]);
  if (s->dp.dbg & 512u)
    fprintf(stderr, "[kr stats] wave cycles/64 per launch: level passes %u, finalize %u, whole read %u\n", hc[kCtCycLevel], hc[kCtCycFinalize], hc[kCtCycRead]);
  if (KR_STATS && (s->dp.dbg & 512u)) { // the accumulate kernel's histograms (g_kr_stats), printed and cleared
    uint32_t hs[128], zero[128] = {0};
    if (hipMemcpyFromSymbol(hs, HIP_SYMBOL(g_kr_stats), sizeof(hs)) == hipSuccess && hipMemcpyToSymbol(HIP_SYMBOL(g_kr_stats), zero, sizeof(zero)) == hipSuccess) {
      auto row = [&](const char* what, int a, int b) {
        fprintf(stderr, "[kr stats] %s:", what);
        for (int i = a; i < b; ++i)
          if (hs[i]) fprintf(stderr, " [%d]=%u", i - a, hs[i]);
        fprintf(stderr, "\n");
      };
      row("reads by log2(events+1)", 0, 32);
      row("reads by log2(marked keys+1)", 32, 64);
      row("reads by log2(records+1)", 64, 96);
      row("paths (0 fast, 1 general, 2 aside:events, 3 aside:tables; the rest: kr_debug_acc_paths)", 96, 100);
      row("records by min(9, events counted)", 110, 120);
    }
  }
  if (int prc = item_placement_step(s)) return prc;
  s->batch.nrecs = extent; // record slots of the device view, unused ones (rec_key == 0) included
  s->batch.nhits = std::min<uint64_t>(hc[kCtTapHits], s->hit_cap);
  // (a tiled batch: the tiles' own records became holes when their sequences' records were written: kCtTileHoles; what survives
  //  is what the caller's max_records bounds)
  const uint32_t recs = hc[kCtRecords], holes = s->batch.tiled ? hc[kCtTileHoles] : 0u;
  if (recs - std::min(recs, holes) > s->rec_user_cap)
    s->batch.rc = kr::fail(KR_ERR_CAPACITY, "the batch produced more records than max_records: submit fewer reads per batch");
  else
    s->batch.rc = check_errflags(hc[kCtErr] | (lane_full ? kErrRecCap : 0u));
  if (s->batch.rc) s->batch.msg = kr_last_error();
  if (!s->batch.rc && s->batch.tiled && getenv("KR_DEBUG_TILE_OVERFLOW")) s->batch.rc = KR_ERR_CAPACITY; // (tests)
  // KR_ROWS_INDEXED (one lane): list positions are handed out up to rep_cap, dist_list holds dist_cap of them
  s->batch.ndist = s->batch.rows_indexed ? std::min<uint64_t>(hc[kCtProblems], s->lanes[0].out.dist_cap) : 0;
  if (s->batch.rows_indexed) s->ix_extent = hc[kCtProblems];
  if (!s->batch.rc && s->batch.rows_indexed && hc[kCtProblems] > s->lanes[0].out.dist_cap) {
    // some row's position may lie beyond the list: the batch again with the hint ignored -- rows with rec_d, as the header promises
    // for a hint that is not honoured (the caller's buffers are still valid, as for the tiled rerun below)
    ++s->ix_fallbacks;
    return rerun_batch(s, &BatchOrigin::unindexed);
  }
  // the tiles' records did not fit: the batch again, one wave per sequence (the caller's buffers are still valid)
  if (s->batch.rc == KR_ERR_CAPACITY && s->batch.tiled) return rerun_batch(s, &BatchOrigin::untiled);
  return s->batch.rc;
}

static void fill_view(kr_stream* s, kr_result_view* v, bool device)
{
  memset(v, 0, sizeof(*v));
  v->nreads = s->batch.nreads;
  v->nrecs = s->batch.nrecs;
  const bool rows_only = (s->batch.flags & KR_ROWS_ONLY) != 0;
  if (device) {
    const BatchOut ro = result_out(s, s->out); // (a tiled batch: the real reads' per-read results)
    v->read_off = ro.rd_off, v->read_cnt = ro.rd_cnt, v->read_onmers = ro.rd_onmers, v->read_na = ro.rd_na;
    v->rec_key = s->out.rec_key, v->rec_sel = s->out.rec_sel, v->rec_d = s->batch.rows_indexed ? nullptr : s->out.rec_d; // (indexed rows lie in rec_d)
    // ... and DIST of record slot i is dist_list[rec_dix[i]]: the select kernels left every selected record's list position in rec_rep
    if (s->batch.rows_indexed) v->rec_dix = s->out.rec_rep, v->dist_list = s->lanes[0].out.dist_list, v->ndist = s->batch.ndist;
    v->rec_v = (rows_only && !(s->batch.flags & KR_TAP_ACCS) && !(!s->dp.no_filter && s->dp.multi)) ? nullptr : s->out.rec_v; // not written then
    v->rec_chisq = (!s->dp.no_filter && s->dp.multi) ? s->out.rec_chisq : nullptr; // written in filter mode only
    // planes exist for every record only in batches that keep histograms (else only where the packed word cannot hold the problem)
    v->rec_hist = (s->batch.flags & KR_TAP_ACCS) ? s->out.rec_hist : nullptr;
    v->rec_hist_stride = (s->batch.flags & KR_TAP_ACCS) ? s->rec_cap : 0;
  } else {
    v->read_off = s->h_rd_off, v->read_cnt = s->h_rd_cnt, v->read_onmers = s->h_rd_onmers, v->read_na = s->h_rd_na;
    v->rec_key = s->h_rec_key.get(), v->rec_sel = s->h_rec_sel.get(), v->rec_d = s->h_rec_d.get();
    if (s->batch.rows_indexed) v->rec_d = nullptr, v->rec_dix = s->h_rec_dix.get(), v->dist_list = s->h_dist_list.get(), v->ndist = s->batch.h_ndist;
    v->rec_v = rows_only ? nullptr : s->h_rec_v.get();
    v->rec_chisq = rows_only ? nullptr : s->h_rec_chisq.get();
    v->rec_hist = (s->batch.flags & KR_TAP_ACCS) && !rows_only ? s->h_rec_hist.get() : nullptr;
    v->rec_hist_stride = s->batch.nrecs;
  }
}

// ---- kr_batch_collect in three pieces: room on the host, one lane's copies, the offsets and the row count ----

static bool collect_full(const kr_stream* s) { return !(s->batch.flags & KR_ROWS_ONLY); }
// what a lane brings back: compact rows -- (key, DIST) per output row, every one selected -- or its record slots
static uint64_t lane_count(const kr_stream* s, const Lane& L) { return s->batch.rows_mode ? L.nrows : L.nrecs; }
static uint64_t batch_count(const kr_stream* s)
{
  uint64_t total = 0;
  for (uint32_t l = 0; l < s->batch.nlanes; ++l) total += lane_count(s, s->lanes[l]);
  return total;
}

// Room for `need` records (rows) in the page-locked record arrays
static int collect_room(kr_stream* s, uint64_t need)
{
  const bool full = collect_full(s);
  const uint64_t have = s->h_rec_key.size();
  if (need <= have && (s->h_rec_full || !full) && (s->h_rec_dix.get() || !s->batch.rows_indexed)) return KR_OK;
  const uint64_t cap = std::max<uint64_t>(std::max<uint64_t>(need + need / 4, have), 1u << 16);
  // all of them anew, every old one freed first (v / chisq / hist stay empty until a batch asks for them, dix until an indexed one
  // does); a failure leaves none behind, and the next collect starts over
  auto drop = [&] { s->h_rec_key.reset(), s->h_rec_sel.reset(), s->h_rec_d.reset(), s->h_rec_hist.reset(), s->h_rec_v.reset(), s->h_rec_chisq.reset(); };
  drop();
  s->h_sel_ones = 0;
  bool ok = s->h_rec_key.renew(cap) && s->h_rec_sel.renew(cap) && s->h_rec_d.renew(cap);
  s->h_rec_dix.reset();
  if (ok && s->batch.rows_indexed) ok = s->h_rec_dix.renew(cap);
  if (ok) s->h_rec_full = s->h_rec_full || full;
  if (ok && s->h_rec_full) ok = s->h_rec_hist.renew(cap * s->dp.np) && s->h_rec_v.renew(cap) && s->h_rec_chisq.renew(cap);
  if (ok) return KR_OK;
  drop(), s->h_rec_dix.reset();
  return alloc_failed("kr_batch_collect: page-locked record arrays");
}

// The copies of lane L, queued on its stream: its records (rows) land at `hoff` in the compact host arrays, the per-read results at
// the lane's reads, read through result_out: a tiled batch is one lane, and its per-read results are the real reads'
static int collect_lane(kr_stream* s, Lane& L, uint64_t hoff)
{
  Batch& b = s->batch;
  hipStream_t st = L.stream;
  const BatchOut o = result_out(s, L.out);
  const bool full = collect_full(s);
  const uint64_t nr = b.tiled ? b.nreads : L.nreads, nc = lane_count(s, L), r0 = L.read0;
  L.host_off = hoff;
  if (b.rows_mode) { // 12 bytes per output row and the reads' row ranges: nothing else crosses PCIe
    HIP_TRY(hipMemcpyAsync(s->h_rd_off + r0, o.rd_roff, nr * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(s->h_rd_cnt + r0, o.rd_rcnt, nr * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(s->h_rd_na + r0, o.rd_na, nr, hipMemcpyDeviceToHost, st));
    s->d2h_bytes += nr * 9;
    if (b.rows_indexed) b.h_ndist = nc ? b.ndist : 0; // (a batch without rows brings no list back)
    if (nc && b.rows_indexed) { // (one lane, waited for: kr_batch_wait has set ndist)
      const uint64_t nd = b.ndist;
      if (nd > s->h_dist_list.size() && !s->h_dist_list.reserve(nd + nd / 4 + 1024)) return alloc_failed("kr_batch_collect: list of distinct DIST values");
      HIP_TRY(hipMemcpyAsync(s->h_rec_key.get() + hoff, o.row_key, nc * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(s->h_rec_dix.get() + hoff, o.row_dix, nc * 4, hipMemcpyDeviceToHost, st));
      if (nd) HIP_TRY(hipMemcpyAsync(s->h_dist_list.get(), o.dist_list, nd * 8, hipMemcpyDeviceToHost, st));
      s->d2h_bytes += nc * 8 + nd * 8;
    } else if (nc) {
      HIP_TRY(hipMemcpyAsync(s->h_rec_key.get() + hoff, o.row_key, nc * 4, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(s->h_rec_d.get() + hoff, o.row_d, nc * 8, hipMemcpyDeviceToHost, st));
      s->d2h_bytes += nc * 12;
    }
    return KR_OK;
  }
  HIP_TRY(hipMemcpyAsync(s->h_rd_off + r0, o.rd_off, nr * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(s->h_rd_cnt + r0, o.rd_cnt, nr * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(s->h_rd_na + r0, o.rd_na, nr, hipMemcpyDeviceToHost, st));
  s->d2h_bytes += nr * 9;
  if (full) {
    HIP_TRY(hipMemcpyAsync(s->h_rd_onmers + r0, o.rd_onmers, nr * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(s->h_rd_filt + 2 * r0, o.rd_filt, nr * 8, hipMemcpyDeviceToHost, st));
    s->d2h_bytes += nr * 12;
  }
  if (!nc) return KR_OK;
  s->h_sel_ones = 0; // (real flags from here on)
  s->d2h_bytes += nc * 13; // key, flag, DIST of every record slot
  HIP_TRY(hipMemcpyAsync(s->h_rec_key.get() + hoff, o.rec_key, nc * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(s->h_rec_sel.get() + hoff, o.rec_sel, nc, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(s->h_rec_d.get() + hoff, o.rec_d, nc * 8, hipMemcpyDeviceToHost, st));
  if (!full) return KR_OK;
  HIP_TRY(hipMemcpyAsync(s->h_rec_v.get() + hoff, o.rec_v, nc * 8, hipMemcpyDeviceToHost, st));
  s->d2h_bytes += nc * 8;
  if (!s->dp.no_filter && s->dp.multi) {
    HIP_TRY(hipMemcpyAsync(s->h_rec_chisq.get() + hoff, o.rec_chisq, nc * 8, hipMemcpyDeviceToHost, st));
    s->d2h_bytes += nc * 8;
  } else
    std::fill(s->h_rec_chisq.get() + hoff, s->h_rec_chisq.get() + hoff + nc, std::numeric_limits<double>::quiet_NaN());
  if (b.flags & KR_TAP_ACCS) { // (waited for: the planes are laid out by the total record count)
    uint64_t hist_stride_host = 0;
    for (uint32_t l = 0; l < b.nlanes; ++l) hist_stride_host += s->lanes[l].nrecs;
    for (uint32_t x = 0; x < s->dp.np; ++x) {
      HIP_TRY(hipMemcpyAsync(s->h_rec_hist.get() + (uint64_t)x * hist_stride_host + hoff, o.rec_hist + (uint64_t)x * s->rec_cap, nc * 4, hipMemcpyDeviceToHost, st));
      s->d2h_bytes += nc * 4;
    }
  }
  return KR_OK;
}

// The copies have landed, `total` records (rows) in all: the reads' offsets from the stream's arrays (lane slices) to the compact
// host arrays, the host view and its number of output rows
static void collect_finish(kr_stream* s, uint64_t total, kr_result_view* v)
{
  const bool rows_mode = s->batch.rows_mode;
  for (uint32_t l = 0; l < s->batch.nlanes; ++l) {
    const Lane& L = s->lanes[l];
    const uint32_t delta = rows_mode ? (uint32_t)L.host_off : (uint32_t)L.host_off - L.rec_base; // (mod 2^32; a lane's rows are numbered from 0)
    if (!delta) continue;
    uint32_t* off = s->h_rd_off + L.read0;
    const uint32_t* cnt = s->h_rd_cnt + L.read0;
    for (uint32_t r = 0; r < L.nreads; ++r) off[r] = cnt[r] ? off[r] + delta : 0u;
  }
  fill_view(s, v, false);
  v->nrecs = (uint32_t)total;
  v->rec_hist_stride = total;
  if (rows_mode) { // every row is an output row: the flags are a block of ones that is written once and kept
    if (s->h_sel_ones < total) {
      const uint64_t a0 = s->h_sel_ones, len = total - a0;
      const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::min(kr::parallel_width(), 16), len >> 22));
      kr::parallel_for(nt, [&](int t) {
        const uint64_t a = a0 + len * (uint64_t)t / nt, b = a0 + len * (uint64_t)(t + 1) / nt;
        memset(s->h_rec_sel.get() + a, 1, b - a);
      });
      s->h_sel_ones = total;
    }
    v->nrows = total;
  } else { // number of output rows: tens of millions of flags for a large batch, summed by the host pool
    const int nt = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)std::min(kr::parallel_width(), 16), total >> 20));
    std::vector<uint64_t> part((size_t)nt, 0);
    const uint8_t* sel = s->h_rec_sel.get();
    kr::parallel_for(nt, [&](int t) {
      uint64_t a = total * (uint64_t)t / nt, b = total * (uint64_t)(t + 1) / nt, c = 0;
      for (uint64_t i = a; i < b; ++i) c += sel[i];
      part[(size_t)t] = c;
    });
    uint64_t nrows = 0;
    for (uint64_t c : part) nrows += c;
    v->nrows = nrows;
  }
}

int kr_batch_collect(kr_stream* s, kr_result_view* v)
{
  kr::clear_error();
  if (!s || !v) return kr::fail(KR_ERR_ARG, "kr_batch_collect: null argument");
  Batch& b = s->batch;
  if (!b.submitted) return kr::fail(KR_ERR_STATE, "kr_batch_collect: nothing submitted");
  if (b.seek) return kr::fail(KR_ERR_STATE, "kr_batch_collect: the batch is a seek batch: kr_batch_collect_seek / kr_batch_collect_text");
  HIP_TRY(hipSetDevice(s->ix->device));
  const bool pipelined = !b.waited && !b.collected;
  s->d2h_bytes = 0;
  static const bool timing = getenv("KR_COLLECT_TIMING") != nullptr;
  auto wall = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  double t_mark = timing ? wall() : 0.0;
  auto lap = [&](const char* what) {
    if (!timing) return;
    const double now = wall();
    fprintf(stderr, "[collect] %s %.2f ms\n", what, (now - t_mark) * 1e3);
    t_mark = now;
  };
  if (!pipelined || b.nlanes == 1 || (b.flags & KR_TAP_ACCS)) {
    int rc = kr_batch_wait(s); // (the histogram planes are laid out by the total record count: it must be known first)
    if (rc) return rc;
  }
  lap("wait for the kernels");
  if (b.waited)
    if (int rc = collect_room(s, batch_count(s))) return rc;
  // Lane by lane: as soon as a lane's kernels are done its results start their way to the host on the lane's own
  // stream, while later lanes still compute.  The host arrays are compact (no unused slots between lanes), so a lane's
  // records land behind those of the lanes before it.
  uint64_t hoff = 0;
  for (uint32_t l = 0; l < b.nlanes; ++l) {
    Lane& L = s->lanes[l];
    if (!b.waited) {
      HIP_TRY(hipStreamSynchronize(L.stream));
      L.nrecs = std::min(L.h_counters[kCtRecSlots], L.rec_cap);
      L.nrows = L.h_counters[kCtRows];
      // room for this lane and, by its measure, for the lanes still running; if not, everything is waited for and the room made
      const uint64_t nc = lane_count(s, L), guess = hoff + nc * (b.nlanes - l) + nc / 8 * (b.nlanes - l - 1);
      if (guess > s->h_rec_key.size() || (collect_full(s) && !s->h_rec_full)) {
        for (uint32_t j = 0; j < b.nlanes; ++j) HIP_TRY(hipStreamSynchronize(s->lanes[j].stream));
        int rc = kr_batch_wait(s);
        if (rc) return rc;
        if ((rc = collect_room(s, batch_count(s)))) return rc;
        hoff = 0; // the buffers moved: the copies of the lanes before this one start over (once: the batch is waited for now)
        for (uint32_t j = 0; j < l; ++j) {
          if ((rc = collect_lane(s, s->lanes[j], hoff))) return rc;
          hoff += lane_count(s, s->lanes[j]);
        }
      }
    }
    if (int rc = collect_lane(s, L, hoff)) return rc;
    hoff += lane_count(s, L);
  }
  if ((b.flags & KR_TAP_HITS) && b.waited && b.nhits)
    HIP_TRY(hipMemcpyAsync(s->h_hits.get(), s->out.hits, b.nhits * sizeof(kr_hit), hipMemcpyDeviceToHost, s->lanes[0].stream));
  int rc = kr_batch_wait(s); // (a no-op when it already ran; otherwise every lane is idle by now: aggregates the counters)
  for (uint32_t l = 0; l < b.nlanes; ++l) HIP_TRY(hipStreamSynchronize(s->lanes[l].stream));
  if (rc) return rc;
  lap("copies to the host");
  b.collected = true;
  collect_finish(s, hoff, v);
  lap("offsets + row count");
  return KR_OK;
}

int kr_batch_collect_device(kr_stream* s, kr_result_view* v)
{
  kr::clear_error();
  if (!s || !v) return kr::fail(KR_ERR_ARG, "kr_batch_collect_device: null argument");
  if (s->batch.submitted && s->batch.seek) return kr::fail(KR_ERR_STATE, "kr_batch_collect_device: the batch is a seek batch: kr_batch_collect_seek");
  int rc = kr_batch_wait(s);
  if (rc) return rc;
  fill_view(s, v, true);
  return KR_OK;
}

int kr_batch_hits(kr_stream* s, const kr_hit** hits, uint64_t* nhits)
{
  if (!s || !hits || !nhits || !s->batch.waited) return kr::fail(KR_ERR_STATE, "kr_batch_hits: collect a KR_TAP_HITS batch first");
  *hits = s->h_hits.get();
  *nhits = s->batch.nhits;
  return KR_OK;
}

int kr_batch_readtaps(kr_stream* s, const kr_readtap** taps)
{
  if (!s || !taps || !s->batch.waited) return kr::fail(KR_ERR_STATE, "kr_batch_readtaps: collect a batch first");
  *taps = reinterpret_cast<const kr_readtap*>(s->h_rd_filt);
  return KR_OK;
}

// Experiments on the scan kernel's launch-time levels (DESIGN.md section 3.1b): give ONE group of the stream's buffers a new
// address (the old buffer stays allocated until the stream is destroyed, so the new one lands elsewhere) or lane 0 a new HIP
// stream.  0: item list; 1: per-read arrays; 2: counters + cursors; 3: records, de-duplication table; 4: HIP stream.
int kr_debug_stream_move(kr_stream* s, int which)
{
  if (!s || (s->batch.submitted && !s->batch.waited)) return kr::fail(KR_ERR_STATE, "kr_debug_stream_move: wait for the batch first");
  HIP_TRY(hipSetDevice(s->device));
  BatchOut& o = s->out;
  Lane& L = s->lanes[0];
  const uint64_t mr = s->max_reads, ML = s->max_lanes;
  int rc = 0;
#define MV(ptr, n)   if ((rc = salloc(s, &ptr, (n)))) return rc;
  switch (which) {
    case 0: MV(o.items, s->item_cap); break;
    case 1:
      MV(o.rd_off, mr); MV(o.rd_cnt, mr); MV(o.rd_onmers, mr); MV(o.rd_filt, 2 * mr); MV(o.rd_na, mr);
      MV(o.rd_it_off, mr); MV(o.rd_it_cnt, mr); MV(o.long_list, mr + 16ull * s->nwaves * ML);
      break;
    case 2: MV(L.d_counters, kCounterWords); MV(L.d_cursors, kCurSets * kCursors * kCursorStride); break;
    case 3:
      MV(o.rec_read, s->rec_cap); MV(o.rec_key, s->rec_cap); MV(o.rec_d, s->rec_cap); MV(o.rec_sel, s->rec_cap);
      MV(o.rec_w0, s->rec_cap); MV(o.rec_rep, s->rec_cap); MV(o.rep_list, (uint64_t)s->rec_cap + (uint64_t)kMaxLanes * kRepSlack); MV(o.rep_dv, (uint64_t)s->rec_cap + (uint64_t)kMaxLanes * kRepSlack);
      MV(L.d_dd, L.dd_slots);
      break;
    case 4: {
      hipStream_t st = nullptr;
      HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
      s->moved_streams.push_back(L.stream);
      L.stream = st;
      break;
    }
    default: return kr::fail(KR_ERR_ARG, "kr_debug_stream_move: which = 0 .. 4");
  }
#undef MV
  return KR_OK;
}

// (experiments) device addresses of the buffers the scan kernel touches: item list, counters, cursors, rd_off, rd_it_off, rd_filt, rec_key, dedup table
int kr_debug_stream_addrs(kr_stream* s, uint64_t* out8)
{
  if (!s || !out8) return kr::fail(KR_ERR_ARG, "kr_debug_stream_addrs: null argument");
  const BatchOut& o = s->out;
  const Lane& L = s->lanes[0];
  const void* p[8] = {o.items, L.d_counters, L.d_cursors, o.rd_off, o.rd_it_off, o.rd_filt, o.rec_key, L.d_dd};
  for (int i = 0; i < 8; ++i) out8[i] = (uint64_t)(uintptr_t)p[i];
  return KR_OK;
}

int kr_debug_item_placement(kr_stream* s, uint32_t* tried, uint32_t* kept, double* best_ns_per_read)
{
  if (!s) return kr::fail(KR_ERR_ARG, "kr_debug_item_placement: null argument");
  if (tried) *tried = s->ipl.tried;
  if (kept) *kept = s->ipl.kept_new;
  if (best_ns_per_read) *best_ns_per_read = s->ipl.best_ns;
  return KR_OK;
}

// (tests) KR_ROWS_INDEXED: list positions the last indexed launch handed out (counters[kCtProblems]; of the first attempt if the batch
// was then run again with rec_d) and how many batches of this stream were run again so
int kr_debug_indexed_list(kr_stream* s, uint64_t* extent, uint64_t* fallbacks)
{
  kr::clear_error();
  if (!s) return kr::fail(KR_ERR_ARG, "kr_debug_indexed_list: null argument");
  if (extent) *extent = s->ix_extent;
  if (fallbacks) *fallbacks = s->ix_fallbacks;
  return KR_OK;
}

// (tests, no device needed) The constants of the select and row kernels (kr_dev_likelihood.inc) that decide which form a read of n
// records takes.  kSelectLaneMax, KR_SELECT_GL and kRowBlock are the kernels' own; the others are literals there -- the ballots of
// kr_select_lane_kernel (n <= 16, n <= 32), select_big_read (n <= 256: registers; t0 += 128: its second pass), kr_rows_write_kernel
// (U = 4 reads for each of the workgroup's four waves) -- and are restated here.
int kr_debug_select_layout(uint32_t* out8)
{
  kr::clear_error();
  if (!out8) return kr::fail(KR_ERR_ARG, "kr_debug_select_layout: null argument");
  out8[0] = kSelectLaneMax, out8[1] = 16, out8[2] = 32, out8[3] = KR_SELECT_GL, out8[4] = 256, out8[5] = 128, out8[6] = kRowBlock, out8[7] = 16;
  return KR_OK;
}

// what kr_debug_select requires of its tables, given the limits of a stream (kr_debug_select_check: the same without one)
static int select_check(const kr_select_tables* in, uint32_t max_reads, uint64_t max_records, uint32_t nnodes, uint32_t hdist_th, uint32_t places)
{
  auto bad = [](const char* what) { return kr::fail(KR_ERR_ARG, std::string("kr_debug_select: ") + what); };
  const uint32_t nreads = in->nreads, nrecs = in->nrecs;
  if (nreads == 0 || nreads > max_reads) return bad("nreads out of range for this stream");
  if (nrecs > max_records) return bad("more records than the stream's max_records");
  if (!in->rd_off || !in->rd_cnt || !in->rd_onmers) return bad("null read table");
  if (nrecs && (!in->rec_key || !in->rec_rep || !in->rec_w0)) return bad("null record table");
  if ((in->rec_hist == nullptr) != (in->rec_read == nullptr)) return bad("rec_hist and rec_read come together");
  if (in->nrep > max_records || in->problems > in->nrep || (in->nrep && !in->rep_dv)) return bad("list of distinct problems out of range");
  if (in->ndirect > places || (in->ndirect && (!in->dd_direct || !in->dd_dv))) return bad("direct places out of range");
  uint64_t end = 0;
  for (uint32_t r = 0; r < nreads; ++r) {
    const uint64_t o = in->rd_off[r], n = in->rd_cnt[r];
    if (o < end || o + n > nrecs) return bad("read ranges overlap, descend or leave the records");
    end = o + n;
    for (uint64_t i = o; i < o + n; ++i) {
      const uint32_t key = in->rec_key[i], rep = in->rec_rep[i];
      if (i > o && key <= in->rec_key[i - 1]) return bad("keys of a read do not ascend strictly");
      if ((key >> 1) >= nnodes) return bad("key beyond the index's nodes");
      if (rep == 0xFFFFFFFFu) return bad("hole inside a read");
      if (rep & kDdDirectFlag) {
        const uint32_t pl = rep & ~kDdDirectFlag;
        if (pl >= in->ndirect || in->dd_direct[pl] >= in->nrep) return bad("direct place out of range");
      } else if (rep >= in->nrep) {
        return bad("list position out of range");
      }
      if (in->rec_w0[i] != 0 ? hdist_th != 4 : (!in->rec_hist || in->rec_read[i] != r)) return bad("record without a problem");
    }
  }
  return KR_OK;
}
int kr_debug_select_check(const kr_select_tables* in, uint32_t max_reads, uint64_t max_records, uint32_t nnodes, uint32_t hdist_th, uint32_t direct_nodes)
{
  kr::clear_error();
  if (!in) return kr::fail(KR_ERR_ARG, "kr_debug_select_check: null argument");
  if (direct_nodes > (1u << 20)) return kr::fail(KR_ERR_ARG, "kr_debug_select_check: direct_nodes out of range");
  return select_check(in, max_reads, max_records, nnodes, hdist_th, kDdOslots * kDdClasses * direct_nodes);
}
// (tests) Crafted records through the select and row kernels as a one-lane batch submitted with `flags` would run them: the lane's view
// is set_lane_view's, the launches are launch_select's and launch_rows'.  Everything the kernels may read is checked first: a table that
// passes cannot send them outside the stream's buffers.
int kr_debug_select(kr_stream* s, const kr_select_tables* in, uint32_t flags, uint32_t form, kr_select_result* out)
{
  kr::clear_error();
  if (!s || !in || !out) return kr::fail(KR_ERR_ARG, "kr_debug_select: null argument");
  if (s->max_lanes != 1 || (s->batch.submitted && !s->batch.waited)) return kr::fail(KR_ERR_STATE, "kr_debug_select: needs an idle one-lane stream");
  auto bad = [](const char* what) { return kr::fail(KR_ERR_ARG, std::string("kr_debug_select: ") + what); };
  if (form > 1) return bad("form is 0 or 1");
  if (flags != 0 && flags != KR_TAP_ACCS && flags != KR_ROWS_ONLY && flags != (KR_ROWS_ONLY | KR_ROWS_INDEXED)) return bad("unsupported flags");
  if (int rc = select_check(in, s->max_reads, std::min<uint64_t>(s->rec_user_cap, s->rec_cap), s->ix->dix.libs[0].nnodes, s->llh.th, kDdOslots * kDdClasses * s->out.dd_nodes))
    return rc;
  const uint32_t nreads = in->nreads, nrecs = in->nrecs, np = s->dp.np;
  HIP_TRY(hipSetDevice(s->device));
  Lane& L = s->lanes[0];
  hipStream_t st = L.stream;
  begin_batch(s, nullptr, nullptr, nreads, flags, BatchOrigin{}, false); // (a crafted batch: neither tiled nor text, nothing to wait for)
  set_lanes_and_row_modes(s, 1);
  L.read0 = 0, L.nreads = nreads, L.rec_base = 0, L.rec_cap = s->rec_cap, L.nrecs = nrecs;
  set_lane_view(s, L, 0, 0, flags, s->rec_cap, s->item_cap, s->item_cap, debug_list_caps());
  BatchOut& o = L.out;
  // ---- poison, then the tables (the plain rows alias rec_rep / rep_dv: what is uploaded there stands)
  const uint64_t nr = nrecs;
  HIP_TRY(hipMemsetAsync(o.rd_na, 0xA5, nreads, st));
  HIP_TRY(hipMemsetAsync(o.rd_rcnt, 0xA5, (uint64_t)nreads * 4, st));
  HIP_TRY(hipMemsetAsync(o.rd_roff, 0xA5, (uint64_t)nreads * 4, st));
  if (nr) {
    HIP_TRY(hipMemsetAsync(o.rec_sel, 0xA5, nr, st));
    HIP_TRY(hipMemsetAsync(o.rec_d, 0xA5, nr * 8, st));
    HIP_TRY(hipMemsetAsync(o.rec_v, 0xA5, nr * 8, st));
    HIP_TRY(hipMemsetAsync(o.rec_chisq, 0xA5, nr * 8, st));
    HIP_TRY(hipMemsetAsync(o.row_key, 0xA5, nr * 4, st));
    if (o.rows_indexed) HIP_TRY(hipMemsetAsync(o.row_dix, 0xA5, nr * 4, st));
    else HIP_TRY(hipMemsetAsync(o.row_d, 0xA5, nr * 8, st));
  }
  if (o.rows_indexed && in->problems) HIP_TRY(hipMemsetAsync(o.dist_list, 0xA5, (uint64_t)in->problems * 8, st));
  HIP_TRY(hipMemsetAsync(o.counters, 0, kCounterWords * 4, st));
  HIP_TRY(hipMemcpyAsync(o.counters + kCtProblems, &in->problems, 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(o.rd_off, in->rd_off, (uint64_t)nreads * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(o.rd_cnt, in->rd_cnt, (uint64_t)nreads * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(o.rd_onmers, in->rd_onmers, (uint64_t)nreads * 4, hipMemcpyHostToDevice, st));
  std::vector<uint32_t> planes;
  if (nr) {
    HIP_TRY(hipMemcpyAsync(o.rec_key, in->rec_key, nr * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o.rec_rep, in->rec_rep, nr * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o.rec_w0, in->rec_w0, nr * 8, hipMemcpyHostToDevice, st));
    if (in->rec_hist) {
      planes.resize(nr * np);
      for (uint64_t i = 0; i < nr; ++i)
        for (uint32_t x = 0; x < np; ++x) planes[x * nr + i] = in->rec_hist[i * np + x];
      for (uint32_t x = 0; x < np; ++x) HIP_TRY(hipMemcpyAsync(o.rec_hist + x * o.rec_stride, planes.data() + x * nr, nr * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(o.rec_read, in->rec_read, nr * 4, hipMemcpyHostToDevice, st));
    }
  }
  if (in->nrep) HIP_TRY(hipMemcpyAsync(o.rep_dv, in->rep_dv, (uint64_t)in->nrep * 16, hipMemcpyHostToDevice, st));
  if (in->ndirect) {
    HIP_TRY(hipMemcpyAsync(o.dd_direct, in->dd_direct, (uint64_t)in->ndirect * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o.dd_dv, in->dd_dv, (uint64_t)in->ndirect * 16, hipMemcpyHostToDevice, st));
  }
  // ---- the select kernel; the record arrays as it leaves them
  launch_select(s, L, form == 0 ? select_lane_default() : false);
  HIP_TRY(hipGetLastError());
  auto back = [&](void* dst, const void* src, uint64_t bytes) -> hipError_t { return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
  HIP_TRY(back(out->rd_na, o.rd_na, nreads));
  HIP_TRY(back(out->rd_rcnt, o.rd_rcnt, (uint64_t)nreads * 4));
  HIP_TRY(back(out->rec_sel, o.rec_sel, nr));
  HIP_TRY(back(out->rec_d, o.rec_d, nr * 8));
  HIP_TRY(back(out->rec_v, o.rec_v, nr * 8));
  HIP_TRY(back(out->rec_chisq, o.rec_chisq, nr * 8));
  HIP_TRY(back(out->rec_rep, o.rec_rep, nr * 4));
  HIP_TRY(hipStreamSynchronize(st));
  // ---- the rows
  out->nrows = 0;
  out->rows_mode = o.rows_mode, out->rows_indexed = o.rows_indexed, out->keep_v = o.keep_v;
  if (o.rows_mode) {
    launch_rows(s, L);
    HIP_TRY(hipGetLastError());
    uint32_t nrows = 0;
    HIP_TRY(hipMemcpyAsync(&nrows, o.counters + kCtRows, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(back(out->row_key, o.row_key, nr * 4));
    if (o.rows_indexed) {
      HIP_TRY(back(out->row_dix, o.row_dix, nr * 4));
      HIP_TRY(back(out->dist_list, o.dist_list, (uint64_t)in->problems * 8));
    } else {
      HIP_TRY(back(out->row_d, o.row_d, nr * 8));
    }
    HIP_TRY(hipStreamSynchronize(st));
    out->nrows = nrows;
  }
  HIP_TRY(back(out->rd_roff, o.rd_roff, (uint64_t)nreads * 4));
  HIP_TRY(hipStreamSynchronize(st));
  return KR_OK;
}

// (tests, no device needed) The constants the designs of tests/dedup_craft.py depend on, all of them the kernels' own names
// (kr_dev_likelihood.inc): a changed table floor, probe limit, chunk or hash moves the designs or fails tests/test_dedup_craft_cpu.py.
int kr_debug_dedup_layout(uint32_t* out12)
{
  kr::clear_error();
  if (!out12) return kr::fail(KR_ERR_ARG, "kr_debug_dedup_layout: null argument");
  out12[0] = kDdOslots, out12[1] = kDdClasses, out12[2] = kDdMaxEvents, out12[3] = kDdMinSlots, out12[4] = (uint32_t)kDdProbeRounds;
  out12[5] = kRepChunk, out12[6] = kRepChunkMax, out12[7] = kDedupBlocks, out12[8] = kDdOslotReads;
  out12[9] = (uint32_t)kDdHashWord, out12[10] = (uint32_t)(kDdHashWord >> 32), out12[11] = kDdHashLeaf;
  return KR_OK;
}

// what kr_debug_dedup requires of its tables, given the limits of a stream (kr_debug_dedup_check: the same without one).  Every record
// slot is looked at: kr_dedup_kernel walks the slots, not the reads, so a slot outside the reads' ranges must be a hole (key 0)
static int dedup_check(const kr_dedup_tables* in, uint32_t max_reads, uint64_t max_records, uint32_t nnodes, uint32_t hdist_th)
{
  auto bad = [](const char* what) { return kr::fail(KR_ERR_ARG, std::string("kr_debug_dedup: ") + what); };
  const uint32_t nreads = in->nreads, nrecs = in->nrecs;
  if (nreads == 0 || nreads > max_reads) return bad("nreads out of range for this stream");
  if (nrecs > max_records) return bad("more records than the stream's max_records");
  if (!in->rd_off || !in->rd_cnt || !in->rd_onmers) return bad("null read table");
  if (nrecs && (!in->rec_key || !in->rec_w0)) return bad("null record table");
  if ((in->rec_hist == nullptr) != (in->rec_read == nullptr)) return bad("rec_hist and rec_read come together");
  uint64_t end = 0;
  for (uint32_t r = 0; r < nreads; ++r) {
    const uint64_t o = in->rd_off[r], n = in->rd_cnt[r];
    if (o < end || o + n > nrecs) return bad("read ranges overlap, descend or leave the records");
    end = o + n;
  }
  end = 0;
  for (uint32_t r = 0; r < nreads; ++r) {
    const uint64_t o = in->rd_off[r], n = in->rd_cnt[r];
    for (uint64_t i = end; i < o; ++i)
      if (in->rec_key[i] != 0) return bad("record outside the reads' ranges");
    end = o + n;
    for (uint64_t i = o; i < o + n; ++i) {
      const uint32_t key = in->rec_key[i];
      const uint64_t w0 = in->rec_w0[i];
      if (key == 0) return bad("hole (key 0) inside a read");
      if ((key >> 1) >= nnodes) return bad("key beyond the index's nodes");
      if (w0 != 0) {
        if (hdist_th != 4) return bad("packed word at a threshold other than 4");
        if (!(w0 >> 63)) return bad("packed word without bit 63");
        if (((w0 >> 40) & 0xFFFFu) != in->rd_onmers[r]) return bad("packed word whose k-mer count is not its read's");
      } else {
        if (!in->rec_hist) return bad("record without a word and without a histogram");
        if (in->rec_read[i] != r) return bad("rec_read names another read");
      }
    }
  }
  for (uint64_t i = end; i < nrecs; ++i)
    if (in->rec_key[i] != 0) return bad("record outside the reads' ranges");
  return KR_OK;
}
int kr_debug_dedup_check(const kr_dedup_tables* in, uint32_t max_reads, uint64_t max_records, uint32_t nnodes, uint32_t hdist_th)
{
  kr::clear_error();
  if (!in) return kr::fail(KR_ERR_ARG, "kr_debug_dedup_check: null argument");
  return dedup_check(in, max_reads, max_records, nnodes, hdist_th);
}
// (tests) Crafted records through the likelihood de-duplication and the minimisations as a one-lane batch would run them: the lane's
// view is set_lane_view's, the launches are launch_likelihood's.  Everything the kernels may read is checked first: a table that passes
// cannot send them outside the stream's buffers (keys index rho and, below dd_nodes, the direct part; rec_read indexes rd_onmers; the
// k-mer count of a packed word indexes dd_oslot below 256 only; list positions are bounded by rep_cap in the kernels themselves).
// The table is NOT poisoned: what an earlier batch of the stream left beyond this batch's mask stays there, for the kernels to ignore.
int kr_debug_dedup(kr_stream* s, const kr_dedup_tables* in, kr_dedup_result* out)
{
  kr::clear_error();
  if (!s || !in || !out) return kr::fail(KR_ERR_ARG, "kr_debug_dedup: null argument");
  if (s->max_lanes != 1 || (s->batch.submitted && !s->batch.waited)) return kr::fail(KR_ERR_STATE, "kr_debug_dedup: needs an idle one-lane stream");
  if (int rc = dedup_check(in, s->max_reads, std::min<uint64_t>(s->rec_user_cap, s->rec_cap), s->ix->dix.libs[0].nnodes, s->llh.th)) return rc;
  const uint32_t nreads = in->nreads, nrecs = in->nrecs, np = s->dp.np;
  HIP_TRY(hipSetDevice(s->device));
  Lane& L = s->lanes[0];
  hipStream_t st = L.stream;
  begin_batch(s, nullptr, nullptr, nreads, 0, BatchOrigin{}, false); // (a crafted batch: neither tiled nor text, nothing to wait for)
  set_lanes_and_row_modes(s, 1);
  L.read0 = 0, L.nreads = nreads, L.rec_base = 0, L.rec_cap = s->rec_cap, L.nrecs = nrecs;
  set_lane_view(s, L, 0, 0, 0, s->rec_cap, s->item_cap, s->item_cap, debug_list_caps());
  BatchOut& o = L.out;
  const uint64_t nr = nrecs, places = (uint64_t)kDdOslots * kDdClasses * o.dd_nodes, places4 = (places + 3) & ~3ull;
  // ---- poison every output, then the tables
  if (nr) HIP_TRY(hipMemsetAsync(o.rec_rep, 0xA5, nr * 4, st));
  HIP_TRY(hipMemsetAsync(o.rep_list, 0xA5, (uint64_t)o.rep_cap * 4, st));
  HIP_TRY(hipMemsetAsync(o.rep_dv, 0xA5, (uint64_t)o.rep_cap * 16, st));
  if (o.dd_nodes) {
    HIP_TRY(hipMemsetAsync(o.dd_direct, 0xA5, places4 * 4, st));
    HIP_TRY(hipMemsetAsync(o.dd_dv, 0xA5, places4 * 16, st));
    HIP_TRY(hipMemsetAsync(o.dd_ohist, 0xA5, 260 * 4, st));
    HIP_TRY(hipMemsetAsync(o.dd_oslot, 0xA5, 256, st));
  }
  HIP_TRY(hipMemsetAsync(o.counters, 0, kCounterWords * 4, st));
  HIP_TRY(hipMemcpyAsync(o.counters + kCtRecSlots, &in->nrecs, 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(o.rd_off, in->rd_off, (uint64_t)nreads * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(o.rd_cnt, in->rd_cnt, (uint64_t)nreads * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(o.rd_onmers, in->rd_onmers, (uint64_t)nreads * 4, hipMemcpyHostToDevice, st));
  std::vector<uint32_t> planes;
  if (nr) {
    HIP_TRY(hipMemcpyAsync(o.rec_key, in->rec_key, nr * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(o.rec_w0, in->rec_w0, nr * 8, hipMemcpyHostToDevice, st));
    if (in->rec_hist) {
      planes.resize(nr * np);
      for (uint64_t i = 0; i < nr; ++i)
        for (uint32_t x = 0; x < np; ++x) planes[x * nr + i] = in->rec_hist[i * np + x];
      for (uint32_t x = 0; x < np; ++x) HIP_TRY(hipMemcpyAsync(o.rec_hist + x * o.rec_stride, planes.data() + x * nr, nr * 4, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(o.rec_read, in->rec_read, nr * 4, hipMemcpyHostToDevice, st));
    }
  }
  // ---- the stage
  launch_likelihood(s, L);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(L.h_counters, o.counters, kCounterWords * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st)); // (the uploads above come from pageable memory: `planes` may go only now)
  const uint32_t problems = L.h_counters[kCtProblems];
  uint32_t mask = kDdMinSlots; // dd_mask, on the host
  while (mask < o.dd_slots && mask < (std::min(nrecs, o.rec_cap) >> o.dd_shift)) mask <<= 1;
  mask -= 1u;
  out->problems = problems, out->err = L.h_counters[kCtErr], out->rep_cap = o.rep_cap;
  out->places = (uint32_t)places, out->dd_nodes = o.dd_nodes, out->mask = mask, out->dd_slots = o.dd_slots, out->dd_shift = o.dd_shift;
  const uint64_t nlist = std::min<uint64_t>(out->rep_room, o.rep_cap), ntab = std::min<uint64_t>(out->table_room, o.dd_slots);
  out->rep_n = (uint32_t)nlist, out->table_n = (uint32_t)ntab;
  auto back = [&](void* dst, const void* src, uint64_t bytes) -> hipError_t { return (dst && src && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
  HIP_TRY(back(out->rec_rep, o.rec_rep, nr * 4));
  HIP_TRY(back(out->rep_list, o.rep_list, nlist * 4));
  HIP_TRY(back(out->rep_dv, o.rep_dv, nlist * 16));
  const uint64_t npl = std::min<uint64_t>(out->places_room, places);
  HIP_TRY(back(out->dd_direct, o.dd_direct, npl * 4));
  HIP_TRY(back(out->dd_dv, o.dd_dv, npl * 16));
  HIP_TRY(back(out->dd_oslot, o.dd_nodes ? o.dd_oslot : nullptr, 256));
  HIP_TRY(back(out->dd_table, o.dd_table, ntab * 16));
  HIP_TRY(hipStreamSynchronize(st));
  return KR_OK;
}

// (tests) The accumulate kernel's path witnesses of the batch last waited for (KR_DEBUG_SKIP=512; CounterSlot kCtFp* .. kCtRd*, summed
// over the lanes): the first min(n, 21) of them into out.  Returns KR_OK.
int kr_debug_acc_paths(kr_stream* s, uint32_t* out, uint32_t n)
{
  kr::clear_error();
  if (!s || !out) return kr::fail(KR_ERR_ARG, "kr_debug_acc_paths: null argument");
  if (!s->batch.waited) return kr::fail(KR_ERR_STATE, "kr_debug_acc_paths: wait for a batch first");
  for (uint32_t i = 0; i < std::min(n, kCtPathCount); ++i) out[i] = s->h_counters[kCtPathFirst + i];
  return KR_OK;
}

// (tests, no device needed unless `s` is given) The event region of the accumulate instantiation for np = hdist_th + 1 planes, reads of
// `segs` (1, 2) segments or the merge instantiation (multi): out8 = {events in the LDS before a read's events spill (ev_cap), words of
// the region (ev_words), words per key of a batch of finalize_events_fast, number of path witnesses, events / passing-key table
// entries / keys a wave's global scratch holds for `s` (0 without a stream), 0}
int kr_debug_acc_layout(const kr_stream* s, uint32_t np, uint32_t segs, uint32_t multi, uint32_t* out8)
{
  kr::clear_error();
  if (!out8 || np == 0 || np > (uint32_t)kMaxPlanes || segs < 1 || segs > 2) return kr::fail(KR_ERR_ARG, "kr_debug_acc_layout: bad argument");
  const AccLayout l = acc_layout(np, segs, multi != 0);
  out8[0] = l.ev_cap, out8[1] = l.ev_words, out8[2] = kFastKeyWords, out8[3] = kCtPathCount;
  out8[4] = s ? s->out.ev_spill : 0u, out8[5] = s ? s->out.tab_spill : 0u, out8[6] = s ? s->out.kt_spill : 0u, out8[7] = 0;
  return KR_OK;
}

// (tests, no device needed) The numbers of the scan shape with_scan_shape picks for a table of `slot_format` (0: packed, shape by
// log_g; 5..8: slotted; 9: filter slots), the very constants the kernels are instantiated with: out16 = {G lanes per probe, CPL
// chunks per lane and pass, PPS probes per pass, words per slot (0: packed), CAP entries of a slot, step bits of a group before the
// hit chunks are dealt out (packed: scan_group's kBits; slotted: the bits a full list uses), kListCap, kItemStage, kItemChunk,
// kReadChunk, kCursors, kSegPos, codes per line and per slot of format 9 (else 0), 1 if slotted, largest hdist_th of format 9's scan}
int kr_debug_scan_layout(uint32_t slot_format, uint32_t log_g, uint32_t* out16)
{
  kr::clear_error();
  if (!out16 || log_g > 3 || log_g == 1 || (slot_format != 0 && (slot_format < 5 || slot_format > kSlotFilter)))
    return kr::fail(KR_ERR_ARG, "kr_debug_scan_layout: bad argument");
  memset(out16, 0, 16 * sizeof(uint32_t));
  if (slot_format == kSlotFilter) {
    out16[0] = kFiltG, out16[1] = kFiltCpl, out16[2] = kFiltPps, out16[3] = slot_words(kSlotFilter), out16[4] = kFiltSlotCodes;
    out16[5] = (kListCap / kFiltPps) * kFiltCpl, out16[12] = kFiltLineCodes, out16[13] = kFiltSlotCodes, out16[14] = 1;
  } else {
    with_scan_shape(slot_format, log_g, [&](auto LG, auto CP, auto SLOTTED) {
      constexpr uint32_t G = 1u << LG.value, PPS = 64u >> LG.value;
      out16[0] = G, out16[1] = (uint32_t)CP.value, out16[2] = PPS;
      if (SLOTTED.value) {
        out16[3] = scan_slot_words(LG.value, CP.value), out16[4] = scan_slot_cap(LG.value, CP.value);
        out16[5] = (kListCap / PPS) * (uint32_t)CP.value, out16[14] = 1;
      } else {
        out16[5] = scan_step_bits(CP.value);
      }
    });
    if (out16[3] != slot_words(slot_format)) return kr::fail(KR_ERR_STATE, "kr_debug_scan_layout: slot_words() and the scan shape disagree");
  }
  out16[6] = kListCap, out16[7] = kItemStage, out16[8] = kItemChunk, out16[9] = kReadChunk, out16[10] = kCursors, out16[11] = kSegPos;
  out16[15] = kFiltMaxTh;
  return KR_OK;
}

// (tests) What the scan of this stream's batches is: out4 = {1 if kr_scan_pipe_kernel_t is launched (a slotted table, formats 5..8, and
// KR_SCAN_PIPE not 0 when the stream was made), 1 if kr_scan_filt_kernel_t is (format 9 and a threshold its candidates carry), item slots
// a lane's scan may use (KR_DEBUG_ITEM_CAP), item slots the scan of the batch last waited for asked for (kCtItemSlots, over the lanes)}
int kr_debug_scan_stream(const kr_stream* s, uint32_t* out4)
{
  kr::clear_error();
  if (!s || !out4) return kr::fail(KR_ERR_ARG, "kr_debug_scan_stream: null argument");
  const uint32_t f = s->ix->slot_log2w;
  out4[0] = (!s->fk && f >= 5 && f <= 8 && s->scan_pipe) ? 1u : 0u;
  out4[1] = s->fk ? 1u : 0u;
  out4[2] = s->item_cap_dbg ? std::min(s->item_cap, s->item_cap_dbg) : s->item_cap;
  out4[3] = s->batch.waited ? s->h_counters[kCtItemSlots] : 0u;
  return KR_OK;
}

int kr_batch_timing(kr_stream* s, kr_timing* t)
{
  if (!s || !t || !s->batch.waited) return kr::fail(KR_ERR_STATE, "kr_batch_timing: wait for a batch first");
  if (s->batch.seek) return kr::fail(KR_ERR_STATE, "kr_batch_timing: the batch is a seek batch: kr_debug_seek_ms");
  memset(t, 0, sizeof(*t));
  // per phase: the sum over the lanes of the time between the lane's events (with one lane: the kernels' own time;
  // with several, lanes share the chip and the sums exceed ms_total, the span from the first lane's first kernel to the
  // last lane's last)
  float first = 0, last = 0;
  for (uint32_t l = 0; l < s->batch.nlanes; ++l) {
    Lane& L = s->lanes[l];
    float a = 0;
    HIP_TRY(hipEventElapsedTime(&a, L.ev[kEvCopyIn], L.ev[kEvFirstKernel]));
    t->ms_h2d += a;
    HIP_TRY(hipEventElapsedTime(&a, L.ev[kEvFirstKernel], L.ev[kEvScanDone]));
    t->ms_scan += a;
    HIP_TRY(hipEventElapsedTime(&a, L.ev[kEvAccStart], L.ev[kEvAccDone]));
    t->ms_acc += a;
    HIP_TRY(hipEventElapsedTime(&a, L.ev[kEvLlhStart], L.ev[kEvLastKernel]));
    t->ms_llh += a;
    if (l) {
      HIP_TRY(hipEventElapsedTime(&a, s->lanes[0].ev[kEvFirstKernel], L.ev[kEvFirstKernel]));
      first = std::min(first, a);
    }
    HIP_TRY(hipEventElapsedTime(&a, s->lanes[0].ev[kEvFirstKernel], L.ev[kEvLastKernel]));
    last = std::max(last, a);
  }
  t->ms_total = last - first;
  t->lanes = s->batch.nlanes;
  t->overflow_reads = s->h_counters[kCtL2Reads];
  t->stack_spills = s->h_counters[kCtStackSpills];
  return KR_OK;
}

} // extern "C"

// (tests) the tiled form of the batch last submitted, as it lies on the device -- whoever laid it out
int kr_debug_tile_layout(kr_stream* s, uint32_t* nv, uint32_t* nlong, uint64_t* voff, uint8_t* vtile, uint32_t* rfirst, uint32_t* longs, uint8_t* bases)
{
  kr::clear_error();
  if (!s || !nv || !nlong) return kr::fail(KR_ERR_ARG, "kr_debug_tile_layout: null argument");
  *nv = 0, *nlong = 0;
  if (!s->batch.submitted || !s->batch.tiled) return KR_OK;
  const kr_stream::Tiles& t = s->tiles;
  HIP_TRY(hipSetDevice(s->device));
  hipStream_t st = s->lanes[0].stream; // (a tiled batch has one lane: its copies or layout kernels are queued here)
  const uint32_t tnv = s->batch.nv, tnlong = s->batch.nlong;
  *nv = tnv, *nlong = tnlong;
  uint64_t nb = 0;
  HIP_TRY(hipMemcpyAsync(&nb, t.d_voff.get() + tnv, 8, hipMemcpyDeviceToHost, st));
  if (voff) HIP_TRY(hipMemcpyAsync(voff, t.d_voff.get(), ((uint64_t)tnv + 1) * 8, hipMemcpyDeviceToHost, st));
  if (vtile) HIP_TRY(hipMemcpyAsync(vtile, t.d_vtile.get(), tnv, hipMemcpyDeviceToHost, st));
  if (rfirst) HIP_TRY(hipMemcpyAsync(rfirst, t.d_rfirst.get(), (uint64_t)s->batch.nreads * 4, hipMemcpyDeviceToHost, st));
  if (longs) HIP_TRY(hipMemcpyAsync(longs, t.d_longs.get(), (uint64_t)tnlong * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (bases && nb) {
    HIP_TRY(hipMemcpyAsync(bases, t.d_bases.get(), nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return KR_OK;
}

// (tests, no device needed) tile_shape: k-mer positions, tiles and tiled bases of a sequence of `len` bases
int kr_debug_tile_shape(uint64_t len, uint32_t k, uint64_t* nkm, uint64_t* nt, uint64_t* bytes)
{
  kr::clear_error();
  if (!nkm || !nt || !bytes || k == 0) return kr::fail(KR_ERR_ARG, "kr_debug_tile_shape: bad argument");
  const TileShape sh = tile_shape(len, k);
  *nkm = sh.nkm, *nt = sh.nt, *bytes = sh.bytes;
  return KR_OK;
}

// Bytes the last kr_batch_collect copied back to the host: rows or record slots and the per-read arrays (bench.py's host-inclusive
// leg reports them).
int kr_debug_last_d2h_bytes(kr_stream* s, uint64_t* bytes)
{
  kr::clear_error();
  if (!s || !bytes) return kr::fail(KR_ERR_ARG, "kr_debug_last_d2h_bytes: null argument");
  *bytes = s->d2h_bytes;
  return KR_OK;
}
