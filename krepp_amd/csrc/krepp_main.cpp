// krepp_main.cpp — the `krepp` command line: every sub-command of the reference CLI (dist, place, seek, index, sketch,
// inspect).  Option names, defaults, header lines and error conventions follow the reference CLI (src/krepp.cpp:508-712,
// src/krepp.hpp:206-221).
//
// Query pipeline (run_query): reader thread (gz/FASTX, src/rqseq.cpp:180-197) -> workers, each
// GPU with its own replica of the index and each worker with its own kr_stream -> writer emitting
// batches in INPUT order (the reference emits in task-completion order, src/krepp.cpp:368-383).
// Settings: what a run was asked; OutputOrder: who may write when; Run: what the threads share;
// Worker: one stream and the job on it.
#include "krepp_amd.h"

#include <cerrno>
#include <chrono>
#include <cmath>
#include <limits>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <ctime>
#include <deque>
#include <malloc.h>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

#define KREPP_VERSION "v0.8.3"

[[noreturn]] static void error_exit(const std::string& msg)
{ // src/common.cpp:20-24
  fprintf(stderr, "[ERROR] %s\n", msg.c_str());
  exit(EXIT_FAILURE);
}

struct Args {
  std::string sub;
  std::map<std::string, std::string> opt;
  std::map<std::string, bool> flag;
  bool has(const std::string& k) const { return opt.count(k) != 0; }
  std::string get(const std::string& k, const std::string& d = "") const
  {
    auto it = opt.find(k);
    return it == opt.end() ? d : it->second;
  }
};

static const std::map<std::string, std::string> kAlias = {
  {"-i", "--index-dir"}, {"-q", "--query"}, {"-o", "--output-path"}, {"-t", "--nwk-file"}, {"-k", "--kmer-len"},
  {"-w", "--win-len"}, {"-h", "--num-positions"}, {"-m", "--modulo-lsh"}, {"-r", "--residue-lsh"}, {"-l", "--lineage-file"},
};
static const char* kFlags[] = {"--multi", "--filter", "--summarize", "--frac", "--verbose", "--gpu-minimizers", "--gpu-keys", "--gpu-colours", "--tabular", "--gpu-parse", "--gpu-seek", "--gpu-stats", "--bgzf-out", "--gpu-deflate", "--gpu-inflate", "--extract-bgzf", "--interleaved"};

// options as in the reference's CLI (src/krepp.cpp:516-675); the texts are this build's own
static void print_help(const std::string& sub)
{
  const char* query_opts =
    "  -q, --query PATH           query FASTA/FASTQ file (gzip accepted)\n"
    "  -o, --output-path PATH     write the report here [stdout]\n"
    "      --bgzf-out             write the report block-gzipped (BGZF: zcat, bgzip -d, tabix read it; device text is deflated on the GPU)\n"
    "      --bgzf-level N         with --bgzf-out: 1 fixed Huffman codes, 2 dynamic codes, a smaller file for a second coding pass [1]\n"
    "      --bgzf-member N        with --bgzf-out: text bytes a BGZF member takes, 256..65280; shorter members are more and shorter waves on the GPU and a slightly larger file [65280]\n"
    "      --hdist-th N           largest Hamming distance at which a k-mer matches [4]\n";
  const char* index_query_opts =
    "  -i, --index-dir DIR        index directory (as written by `krepp index`, this build's or the reference's)\n"
    "      --chisq X              chi-square threshold of the likelihood-ratio filter [2.706]\n"
    "      --dist-max X           report only distances below X (1e-8 .. 0.33)\n"
    "      --multi / --no-multi   report every reference / edge that passes, or only the best [multi]\n"
    "      --summarize            weighted read counts per reference / edge instead of per-read rows\n"
    "      --gpus N, --device D   GPUs to use (index replicated on each), first device [1, 0]\n";
  const char* build_opts =
    "  -k, --kmer-len N           k-mer length, 19..31\n"
    "  -w, --win-len N            minimizer window (>= k) [k+6]\n"
    "  -h, --num-positions N      LSH positions [k-16]\n"
    "  -m, --modulo-lsh N         modulo partitioning the LSH space [4]\n"
    "  -r, --residue-lsh N        keep k-mers with LSH(x) mod m == r [1]\n"
    "      --frac / --no-frac     keep k-mers with LSH(x) mod m <= r [frac]\n"
    "      --seed N               seed of the random LSH positions\n"
    "      --sdust-t N            sdust score threshold; with --sdust-w > 0 low-complexity intervals stay out of the windows [0: off]\n"
    "      --sdust-w N            sdust window length, >= 4 [0: off]\n";
  printf("krepp (MI355X build, mirrors krepp v0.8.3): dist | place | seek | index | sketch | inspect\n");
  if (sub.empty() || sub == "dist")
    printf("\nkrepp dist -i DIR -q READS: distances of every read to the references it matches\n%s%s"
           "      --filter / --no-filter keep only references not significantly worse than the closest [no-filter]\n"
           "      --gpu-parse            FASTA/FASTQ records found on the GPU (identical output; plain files, and BGZF files, inflated on the GPU; others keep the host reader)\n"
           "      --gpu-inflate          with --gpu-parse: ordinary gzip files are inflated on the GPU too (identical output; without it they keep the host reader)\n",
           query_opts, index_query_opts);
  if (sub.empty() || sub == "place")
    printf("\nkrepp place -i DIR -q READS: placements on the backbone tree (jplace)\n%s%s"
           "  -t, --nwk-file PATH        rooted placement tree (overrides the index's backbone)\n"
           "  -l, --lineage-file PATH    place on the taxonomy of a Greengenes/GTDB style lineage file\n"
           "      --tau N                highest Hamming distance counted by the placement threshold [2]\n"
           "      --filter / --no-filter [filter]\n"
           "      --tabular              tab-separated rows instead of jplace\n"
           "      --gpu-deflate          with --bgzf-out: rows written on the GPU are deflated there, only BGZF members come back (the same text)\n"
           "      --gpu-parse            FASTA/FASTQ records found on the GPU (identical output; plain files, and BGZF files, inflated on the GPU; others keep the host reader)\n"
           "      --gpu-inflate          with --gpu-parse: ordinary gzip files are inflated on the GPU too (identical output; without it they keep the host reader)\n",
           query_opts, index_query_opts);
  if (sub.empty() || sub == "seek")
    printf("\nkrepp seek -i SKETCH -q READS: distance of every read to the one sketched reference\n"
           "  -i, --sketch-path PATH     sketch file (as written by `krepp sketch`)\n%s"
           "      --gpu-parse            FASTA/FASTQ records found on the GPU (identical output; plain files, and BGZF files, inflated on the GPU; others keep the host reader)\n"
           "      --gpu-inflate          with --gpu-parse: ordinary gzip files are inflated on the GPU too (identical output; without it they keep the host reader)\n"
           "      --gpu-seek             seek kernels and report text on the GPU (identical output)\n"
           "      --extract-matched FILE   with --gpu-parse --gpu-seek: the reads whose row carries a DIST, as the exact bytes they have in the input, split on the GPU\n"
           "      --extract-unmatched FILE the other reads (rows with NaN, or above --extract-max); either file or both\n"
           "      --extract-max D        a read is matched only when its DIST is at most D, 0..1 [no limit]\n"
           "      --extract-bgzf         the extract files are BGZF, deflated on the GPU (--bgzf-level and --bgzf-member apply)\n"
           "      --query2 FILE          paired reads: the mates' file (plain FASTQ, record for record with -q); both mates of a pair go to the same part\n"
           "      --output-path2 FILE    with --query2: the report of the mates [not written]\n"
           "      --extract-matched2 FILE   with --query2 and --extract-matched: the matched pairs' mates, record for record with --extract-matched\n"
           "      --extract-unmatched2 FILE with --query2 and --extract-unmatched: the other pairs' mates\n"
           "      --interleaved          paired reads in one file: every pair as two neighbouring records of -q (not with --query2)\n"
           "      --pair-rule any|both   a pair is matched when either mate is, or only when both are [any]\n",
           query_opts);
  if (sub.empty() || sub == "index")
    printf("\nkrepp index -i MAP.tsv -o DIR: build an index (reference ID <tab> FASTA path per line)\n"
           "  -t, --nwk-file PATH        rooted guide tree (default: a balanced tree over the IDs)\n%s"
           "      --num-threads N        CPU threads of the builder [1]\n"
           "      --gpu-minimizers       window minimizers of the genomes on the GPU (identical output)\n"
           "      --gpu-keys             also sort and group all genomes' keys on the GPU (implies --gpu-minimizers; identical output)\n"
           "      --gpu-colours          also find the distinct leaf sets of the keys on the GPU and fold each into a colour once (implies --gpu-keys; identical output)\n"
           "      --device D             the GPU of --gpu-minimizers / --gpu-keys / --gpu-colours [0]\n",
           build_opts);
  if (sub.empty() || sub == "sketch")
    printf("\nkrepp sketch -i GENOME.fa -o SKETCH: sketch of a single FASTA/FASTQ file (default k 26)\n%s"
           "      --gpu-minimizers       window minimizers on the GPU (identical output)\n"
           "      --gpu-keys             also sort the keys and count the rows on the GPU (implies --gpu-minimizers; identical output)\n"
           "      --device D             the GPU of --gpu-minimizers / --gpu-keys [0]\n",
           build_opts);
  if (sub.empty() || sub == "inspect")
    printf("\nkrepp inspect -i DIR: the backbone tree, every partial library's metadata and its colour statistics, on stdout\n"
           "  -i, --index-dir DIR        index directory\n"
           "      --gpu-stats            count the k-mers per colour, the out-degrees and their histograms on the GPU (identical output)\n"
           "      --device D             the GPU of --gpu-stats [0]\n");
  printf("\nEnvironment knobs and what differs from the reference: INTEGRATION.md\n");
}

static Args parse(int argc, char** argv)
{
  Args a;
  for (int i = 1; i < argc; ++i) {
    std::string t = argv[i];
    if (t == "--help" || (t == "-h" && a.sub.empty())) {
      print_help(a.sub);
      exit(0);
    }
    if (t[0] != '-') {
      if (a.sub.empty()) {
        a.sub = t;
        continue;
      }
      error_exit("Unexpected argument: " + t);
    }
    auto al = kAlias.find(t);
    if (al != kAlias.end()) t = al->second;
    bool is_flag = false;
    for (const char* f : kFlags) {
      std::string pos = f, neg = std::string("--no-") + (f + 2);
      if (t == pos || t == neg) {
        a.flag[pos] = (t == pos);
        is_flag = true;
      }
    }
    if (is_flag) continue;
    if (i + 1 >= argc) error_exit("Option " + t + " requires a value");
    a.opt[t] = argv[++i];
  }
  return a;
}


using Clock = std::chrono::steady_clock;
static uint64_t since(Clock::time_point t) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now() - t).count(); }

// `dist` and `place` share everything up to the per-batch back end (src/krepp.cpp:347-394, 434-504); `seek` is a sketch file
// served as a one-leaf index (src/krepp.cpp:321-345, src/seek.cpp).  What a run of them takes from the command line and the
// environment, resolved once (resolve_settings: mode 0 `dist`, 1 `place`, 2 `seek`) before any thread starts:
struct Settings {
  bool place = false, seek = false, summarize = false;
  int tabular = 0; // place: 0 jplace, 1 tabular, 2 summary (--summarize wins over --tabular: src/krepp.cpp:401-405,441,467,493)
  kr_params p, pfront; // (the device front end of `place` keeps every chosen leaf: the place options act in the back end)
  std::string query, index_arg, invocation;
  bool gpu_parse = false; // --gpu-parse asked for (Run::open_input decides whether the file qualifies)
  bool gpu_seek = false;  // seek --gpu-seek: batches flagged KR_SEEK, the report as the device's text
  bool gpu_inflate = false; // --gpu-parse --gpu-inflate: an ordinary gzip file is inflated on the device (kr_gzdev), its records found there
  uint64_t gz_super = 64ull << 20; // KR_GZDEV_SUPER: compressed bytes a super-chunk takes
  uint32_t gz_sub = 32768, gz_ratio = 16; // KR_GZDEV_SUB: bytes a wave searches and decodes from (zlib's blocks are 17-21 KB of FASTQ-like text); KR_GZDEV_RATIO: symbols a compressed byte may inflate to
  uint32_t bgzf_level = 1; // --bgzf-level: the encoder's level, on the workers' streams and in Run::deflated
  uint32_t bgzf_member = 65280; // --bgzf-member: text bytes a member takes, on the workers' streams and in Run::deflated
  bool gpu_deflate = false; // place --bgzf-out --gpu-deflate: kr_stream_place_bgzf on the workers' streams
  bool bgzf_out = false;  // --bgzf-out: every byte of the report goes out as BGZF members (Run::put, Worker::collect)
  // seek --gpu-parse --gpu-seek --extract-matched / --extract-unmatched: the reads split on the device (kr_stream_extract_enable)
  std::string extract_matched, extract_unmatched;
  double extract_max = std::numeric_limits<double>::quiet_NaN(); // --extract-max: NaN = every read with a DIST
  bool extract_bgzf = false;                                     // --extract-bgzf: the two files as BGZF members, deflated on the device
  bool extract() const { return !extract_matched.empty() || !extract_unmatched.empty(); }
  uint32_t extract_which() const { return (extract_matched.empty() ? 0u : KR_EXTRACT_MATCHED) | (extract_unmatched.empty() ? 0u : KR_EXTRACT_UNMATCHED); }
  // paired reads (--query2 FILE or --interleaved): both mates of a pair go to the same part (kr_batch_extract_pair)
  std::string query2, output2, extract_matched2, extract_unmatched2;
  bool interleaved = false;
  uint32_t pair_rule = KR_PAIR_ANY;
  bool paired() const { return !query2.empty() || interleaved; }
  int ngpus = 1, dev0 = 0, wpg = 2, nworkers = 2, write_threads = 4;
  uint32_t max_reads = 0;
  uint64_t batch_bases = 0, max_bases = 0, chunk_bytes = 0, max_records = 0, text_bytes = 0;
  bool timing = false, host_text = false, dev_text = false, serial_write = false, copy_batches = false, clean_exit = false;
  bool plain_dist() const { return !place && !seek && !summarize; }
  // What a submit asks of the front end, per mode.  dist rows / the summary need (leaf, selected, DIST) only: nothing else is copied
  // back (KR_TILE_ROWS: a batch with long sequences, which runs as tiles, has its text written by the device like any other);
  // place keeps its records on the device; seek also reads the k-mer counts.  What is collected: Worker::collect.
  uint32_t rows_flags(bool text_on) const { return place ? KR_TAP_ACCS : seek ? 0u : text_on ? KR_TILE_ROWS : KR_ROWS_ONLY; }
};

static Settings resolve_settings(const Args& a, const std::string& invocation, int mode)
{
  Settings s;
  s.place = mode == 1, s.seek = mode == 2, s.invocation = invocation;
  const bool place = s.place, seek = s.seek;
  s.index_arg = a.has("--index-dir") ? a.get("--index-dir") : a.get("--sketch-path");
  if (!a.has("--query") || s.index_arg.empty()) error_exit("dist/place/seek require -q/--query and -i (index directory or sketch file)");
  if (a.has("--lineage-file") && !place) error_exit("-l/--lineage-file is an option of `place`");
  s.query = a.get("--query");
  s.summarize = !seek && a.flag.count("--summarize") && a.flag.at("--summarize");
  kr_params& p = s.p;
  kr_params_default(&p);
  if (a.has("--hdist-th")) p.hdist_th = (uint32_t)atoi(a.get("--hdist-th").c_str());
  if (a.has("--chisq")) p.chisq = atof(a.get("--chisq").c_str());
  if (a.has("--dist-max")) {
    p.dist_max = atof(a.get("--dist-max").c_str());
    if (!(p.dist_max >= 1e-8 && p.dist_max <= 0.33)) error_exit("--dist-max: value not in range [1e-08, 0.33]");
  }
  if (a.flag.count("--multi")) p.multi = a.flag.at("--multi");
  if (place) p.no_filter = 0; // filter defaults to on for place (src/krepp.cpp:612-615)
  if (s.summarize && !place) p.no_filter = 0, p.multi = 1; // "Overrides --no-multi and --no-filter" (src/krepp.cpp:669-672, src/query.cpp:160-171)
  if (a.flag.count("--filter")) p.no_filter = !a.flag.at("--filter");
  if (a.has("--tau")) p.tau = (uint32_t)atoi(a.get("--tau").c_str());
  if (place && p.hdist_th < p.tau) error_exit("The threshold tau must be less than HD threshold --hdist-th!");
  kr_params_default(&s.pfront);
  s.pfront.hdist_th = p.hdist_th;
  const bool tabular_flag = a.flag.count("--tabular") && a.flag.at("--tabular");
  s.tabular = (place && s.summarize) ? 2 : (tabular_flag ? 1 : 0);
  s.ngpus = std::max(1, a.has("--gpus") ? atoi(a.get("--gpus").c_str()) : 1);
  s.dev0 = a.has("--device") ? atoi(a.get("--device").c_str()) : 0;
  s.gpu_parse = a.flag.count("--gpu-parse") && a.flag.at("--gpu-parse");
  s.gpu_seek = a.flag.count("--gpu-seek") && a.flag.at("--gpu-seek");
  if (s.gpu_seek && !seek) error_exit("--gpu-seek is an option of `seek`");
  s.gpu_inflate = a.flag.count("--gpu-inflate") && a.flag.at("--gpu-inflate");
  if (s.gpu_inflate && !s.gpu_parse) error_exit("--gpu-inflate needs --gpu-parse");
  if (const char* e = getenv("KR_GZDEV_SUPER")) s.gz_super = strtoull(e, nullptr, 10);
  if (const char* e = getenv("KR_GZDEV_SUB")) s.gz_sub = (uint32_t)strtoul(e, nullptr, 10);
  if (const char* e = getenv("KR_GZDEV_RATIO")) s.gz_ratio = (uint32_t)strtoul(e, nullptr, 10);
  s.bgzf_out = a.flag.count("--bgzf-out") && a.flag.at("--bgzf-out");
  s.extract_matched = a.get("--extract-matched"), s.extract_unmatched = a.get("--extract-unmatched");
  s.extract_bgzf = a.flag.count("--extract-bgzf") && a.flag.at("--extract-bgzf");
  if (s.extract() || a.has("--extract-matched") || a.has("--extract-unmatched") || a.has("--extract-max") || s.extract_bgzf) {
    if (!seek) error_exit("--extract-matched, --extract-unmatched, --extract-max and --extract-bgzf are options of `seek`");
    if (!s.gpu_parse || !s.gpu_seek) error_exit("--extract-* needs --gpu-parse and --gpu-seek: the reads are split on the GPU, from the bytes the record finder holds there");
    if (!s.extract()) error_exit("--extract-max and --extract-bgzf need --extract-matched or --extract-unmatched");
    if (a.has("--extract-max")) {
      const std::string v = a.get("--extract-max");
      char* end = nullptr;
      s.extract_max = strtod(v.c_str(), &end);
      if (v.empty() || *end || !(s.extract_max >= 0.0 && s.extract_max <= 1.0)) error_exit("--extract-max: a distance in [0, 1], not " + v);
    }
    if (s.extract_matched == s.extract_unmatched) error_exit("--extract-matched and --extract-unmatched name the same file: " + s.extract_matched);
    if (a.has("--output-path") && (a.get("--output-path") == s.extract_matched || a.get("--output-path") == s.extract_unmatched))
      error_exit("an --extract-* file is also the report's (-o): " + a.get("--output-path"));
  }
  s.query2 = a.get("--query2"), s.output2 = a.get("--output-path2");
  s.extract_matched2 = a.get("--extract-matched2"), s.extract_unmatched2 = a.get("--extract-unmatched2");
  s.interleaved = a.flag.count("--interleaved") && a.flag.at("--interleaved");
  if (a.has("--query2") || a.has("--output-path2") || a.has("--extract-matched2") || a.has("--extract-unmatched2") || a.flag.count("--interleaved") || a.has("--pair-rule")) {
    if (!seek) error_exit("--query2, --output-path2, --extract-matched2, --extract-unmatched2, --interleaved and --pair-rule are options of `seek`");
    if (!s.gpu_parse || !s.gpu_seek || !s.extract())
      error_exit("paired reads (--query2, --interleaved) need --gpu-parse, --gpu-seek and --extract-matched or --extract-unmatched: the pairs are split on the GPU");
    if (a.has("--query2") && s.interleaved) error_exit("--interleaved and --query2 exclude each other: the mates are in a second file or in the same one");
    if (a.has("--query2") && s.query2.empty()) error_exit("--query2: an empty file name");
    for (const char* o : {"--output-path2", "--extract-matched2", "--extract-unmatched2"})
      if (a.has(o) && !a.has("--query2")) error_exit(std::string(o) + " needs --query2");
    if (!s.paired()) error_exit("--pair-rule needs --query2 or --interleaved");
    if (a.has("--pair-rule")) {
      const std::string v = a.get("--pair-rule");
      if (v != "any" && v != "both") error_exit("--pair-rule: any or both, not " + v);
      s.pair_rule = v == "any" ? KR_PAIR_ANY : KR_PAIR_BOTH;
    }
    if (!s.query2.empty()) {
      if (s.extract_matched.empty() != s.extract_matched2.empty())
        error_exit(s.extract_matched2.empty() ? "--extract-matched with --query2 needs --extract-matched2: the mates' file" : "--extract-matched2 needs --extract-matched");
      if (s.extract_unmatched.empty() != s.extract_unmatched2.empty())
        error_exit(s.extract_unmatched2.empty() ? "--extract-unmatched with --query2 needs --extract-unmatched2: the mates' file" : "--extract-unmatched2 needs --extract-unmatched");
      if (s.query2 == s.query) error_exit("--query2 names the same file as -q: " + s.query2);
      const std::string others[] = {a.get("--output-path"), s.extract_matched, s.extract_unmatched};
      const std::string twos[] = {s.output2, s.extract_matched2, s.extract_unmatched2};
      for (size_t x = 0; x < 3; ++x) {
        if (twos[x].empty()) continue;
        bool twice = false;
        for (const std::string& o : others) twice = twice || o == twos[x];
        for (size_t y = 0; y < x; ++y) twice = twice || twos[y] == twos[x];
        if (twice) error_exit("an output file is named twice: " + twos[x]);
      }
    }
  }
  if (a.has("--bgzf-level")) {
    if (!s.bgzf_out && !s.extract_bgzf) error_exit("--bgzf-level needs --bgzf-out");
    const std::string v = a.get("--bgzf-level");
    if (v != "1" && v != "2") error_exit("--bgzf-level: 1 (fixed Huffman codes) or 2 (dynamic codes), not " + v);
    s.bgzf_level = (uint32_t)(v[0] - '0');
  }
  if (a.has("--bgzf-member")) {
    if (!s.bgzf_out && !s.extract_bgzf) error_exit("--bgzf-member needs --bgzf-out");
    const std::string v = a.get("--bgzf-member");
    char* end = nullptr;
    const long m = strtol(v.c_str(), &end, 10);
    if (v.empty() || *end || m < 256 || m > 65280) error_exit("--bgzf-member: 256 to 65280 text bytes a member, not " + v);
    s.bgzf_member = (uint32_t)m;
  }
  if (a.flag.count("--gpu-deflate") && a.flag.at("--gpu-deflate")) {
    if (!place) error_exit("--gpu-deflate is an option of `place`");
    if (!s.bgzf_out) error_exit("--gpu-deflate needs --bgzf-out");
    s.gpu_deflate = !s.summarize; // (--summarize: no rows, nothing to deflate)
  }

  // reads per batch: the kernels' efficiency grows with the batch (launch tails amortise, likelihood problems repeat): 262,144 reads
  // for `dist` on a large input, 65,536 for `place` / `seek` (more state per read) and for inputs of a few batches anyway
  uint32_t max_reads_default = 1u << 16;
  if (!place && !seek) {
    struct stat sb;
    if (stat(s.query.c_str(), &sb) == 0 && S_ISREG(sb.st_mode) && (uint64_t)sb.st_size >= (64ull << 20)) max_reads_default = 1u << 18;
  }
  s.max_reads = getenv("KR_CLI_BATCH_READS") ? (uint32_t)std::max(1, atoi(getenv("KR_CLI_BATCH_READS"))) : max_reads_default;
  s.batch_bases = (uint64_t)s.max_reads * 150, s.max_bases = s.batch_bases * 4;
  // --gpu-parse: about one reader batch of ordinary FASTQ per chunk (2 bytes of input per base); KR_CLI_PARSE_CHUNK (bytes): tests.
  // The chunk is also the longest record the device path takes: a FASTA record longer than a chunk leaves no second record start to
  // cut at, the chunk stops INCOMPLETE with no record, and the host reader takes the file from that record on (docs/design/08)
  s.chunk_bytes = getenv("KR_CLI_PARSE_CHUNK") ? std::max<uint64_t>(4096, strtoull(getenv("KR_CLI_PARSE_CHUNK"), nullptr, 10))
                                               : std::min<uint64_t>(2 * s.batch_bases + (1u << 16), 3ull << 30);
  // two workers (each with its own stream) per GPU: one formats its rows while the other's batch is on the device.  (`place` on a
  // 1000-genome tree, 8 M reads, 65,536-read batches: 8.2 M reads/s with two workers, 7.6 M with three -- `scripts/time_cli_place_big.py`;
  // with 400,000-read batches through the C ABI a third host thread does pay: DESIGN.md 3.4)
  s.wpg = getenv("KR_CLI_WORKERS_PER_GPU") ? std::max(1, atoi(getenv("KR_CLI_WORKERS_PER_GPU"))) : 2;
  s.nworkers = s.ngpus * s.wpg;
  s.max_records = (uint64_t)s.max_reads * (place ? 128 : 64);
  if (const char* e = getenv("KR_DEBUG_CLI_RECORDS")) s.max_records = strtoull(e, nullptr, 10); // tests: force the split-and-retry path
  // device text: room for 1.5 KB of rows per read (33 rows of ~28 bytes on a 1000-genome index); a batch with more is split like one
  // with too many records.  KR_CLI_TEXT_PER_READ (tests): a buffer that is too small
  const char* tpr = getenv("KR_CLI_TEXT_PER_READ");
  s.text_bytes = tpr ? std::max<uint64_t>(4096, (uint64_t)s.max_reads * strtoull(tpr, nullptr, 10)) : std::max<uint64_t>(32ull << 20, (uint64_t)s.max_reads * 1536ull);
  s.write_threads = getenv("KR_CLI_WRITE_THREADS") ? std::max(1, atoi(getenv("KR_CLI_WRITE_THREADS"))) : 4; // (per worker: Worker::emit)
  s.timing = getenv("KR_CLI_TIMING") != nullptr; // seconds spent parsing, on the device (submit + collect), formatting and writing
  // Plain `dist` rows are formatted on the device (kr_batch_submit_text / kr_batch_collect_text: the text of a batch arrives as
  // bytes in the stream's page-locked buffer) and written by the WORKER itself, straight from that buffer, when the batch's turn
  // has come.  KR_CLI_HOST_TEXT=1: the host formatter (kr_format_dist) as before round 5.
  s.host_text = getenv("KR_CLI_HOST_TEXT") != nullptr;
  s.dev_text = s.plain_dist() && !s.host_text;
  s.serial_write = getenv("KR_CLI_SERIAL_WRITE") != nullptr;  // (OutputOrder::open)
  s.copy_batches = getenv("KR_CLI_COPY_BATCHES") != nullptr;  // (Run::read_host)
  s.clean_exit = getenv("KR_CLI_CLEAN_EXIT") != nullptr;      // (Run::finish)
  return s;
}

struct Job {
  uint64_t seq = 0;
  // the batch as views: into a batch the reader handed over whole (kr_fastx_detach: nothing copied, given back by the worker
  // when the batch is done) or into the copies below (a reader batch cut into several jobs)
  const uint8_t* bases = nullptr;
  const uint64_t* offsets = nullptr;  // [n + 1], offsets[0] is the job's first base within `bases`
  const char* const* names = nullptr; // [n] NUL-terminated, back to back in one buffer, in order
  size_t n = 0;
  const char* blob = nullptr;         // = names[0]: the names' buffer
  size_t blob_bytes = 0;
  kr_fastx_held* held = nullptr;
  std::vector<uint8_t> own_bases;
  std::vector<uint64_t> own_offsets;
  std::string own_blob;
  std::vector<const char*> own_names;
  std::string text;
  std::string ex_matched, ex_unmatched; // seek --extract-*: the bytes the two files take from this job, plain or BGZF members
  // paired reads: the mates' chunk (page-locked, --query2), their report rows and their two byte strings
  uint8_t* raw2 = nullptr;
  uint64_t raw2_len = 0, raw2_off = 0;
  bool at_eof2 = false;
  std::string text2, ex_matched2, ex_unmatched2;
  std::vector<kr_placement> pls; // place --summarize: the placements, `read` = global read number
  uint64_t first_read = 0;
  // --gpu-parse: a chunk of the file's raw bytes (page-locked), cut at a guessed record start; its records are found on the device
  uint8_t* raw = nullptr;
  uint64_t raw_len = 0, raw_off = 0;
  bool at_eof = false;
  bool fasta = false, closed = false; // a chunk of a FASTA file (kr_batch_submit_fasta); its last record ends where the chunk does
  // ... of a block-gzipped file: whole members (page-locked) that the device inflates (kr_batch_submit_bgzf); the chunk is bytes
  // [skip, skip + raw_len) of what they hold, and `raw` receives them.  m_off / m_u: every member's offset in the file and its first
  // inflated byte among the job's, with the end of the last member behind them
  uint8_t* comp = nullptr;
  uint64_t comp_len = 0;
  uint32_t skip = 0;
  std::vector<uint64_t> m_off, m_u;
  // chunk position -> BGZF virtual offset (member's file offset << 16 | byte inside the member)
  uint64_t voffset(uint64_t pos) const
  {
    const uint64_t u = skip + pos;
    size_t m = m_u.size() - 1;
    while (m > 0 && m_u[m] > u) --m;
    return m_off[m] << 16 | (u - m_u[m]);
  }
};

// The run's one lock and everything it protects about the ORDER of the output.  Jobs are numbered by the reader; their rows appear
// in that order whoever writes them: a worker in its job's turn (device text; side by side with pwrite when the output is a regular
// file, since a job's place in it is known as soon as the jobs before it know their lengths) or the writer thread from the job's
// text.  `next_seq` is the job the output is waiting for; only the writer advances it, when it has been given that job.
// --gpu-parse: the first chunk (in file order) that stops early names the byte where the host reader takes over for good; chunks
// behind it were handed out already and produce nothing -- the rule lives in dropped_locked() and nowhere else.
// A job that has been given to the writer is gone from the worker: finish() and a whole-job claim() take the unique_ptr.
// (The run's queues borrow `mu` and `cv_work`: their waits also end on an error or an early stop, and one lock keeps that free of
// missed wake-ups.)
class OutputOrder {
public:
  std::mutex mu;
  std::condition_variable cv_work, cv_done;

  // A regular output file is written side by side (one thread copies ~10 GB/s into the page cache: 13 M reads/s of 33 rows each);
  // anything else (a pipe, a terminal) is written in turn.  KR_CLI_SERIAL_WRITE=1: in turn always.
  void open(FILE* out, bool side_by_side)
  {
    struct stat sb;
    if (!side_by_side || out == stdout) return;
    fflush(out);
    if (fstat(fileno(out), &sb) == 0 && S_ISREG(sb.st_mode) && (file_off_ = ftello(out)) >= 0) seekable_ = true;
  }
  void rewind_to_end(FILE* out) const // (when every thread has been joined: the stream continues behind what the workers wrote)
  {
    if (!seekable_) return;
    fflush(out);
    (void)fseeko(out, file_off_, SEEK_SET);
  }

  // Waits for the job's turn.  False: nothing of this job reaches the output (an error, or a chunk behind the first early stop).
  bool wait_turn(const Job& j)
  {
    std::unique_lock<std::mutex> lk(mu);
    return turn(lk, j);
  }
  // The job's turn, and room for `n` bytes of it: *at is their place in the file (pwrite), or -1 (write them now, in turn).
  // whole_job: these are all its rows -- the job goes to the writer here, so that the next job may take its place in the file
  // while this one is being copied, and `j` is empty afterwards.  False: write nothing.
  bool claim(std::unique_ptr<Job>& j, size_t n, bool whole_job, off_t* at)
  {
    std::unique_lock<std::mutex> lk(mu);
    if (!turn(lk, *j)) return false;
    *at = seekable_ ? file_off_ : (off_t)-1;
    if (!seekable_) return true;
    file_off_ += (off_t)n;
    if (whole_job) {
      const uint64_t seq = j->seq;
      finished_[seq] = std::move(j);
      lk.unlock();
      cv_done.notify_all();
    }
    return true;
  }
  void finish(std::unique_ptr<Job> j, std::string& text, std::vector<kr_placement>& pls)
  {
    const uint64_t seq = j->seq;
    j->text.swap(text), j->pls.swap(pls);
    { std::lock_guard<std::mutex> lk(mu); finished_[seq] = std::move(j); }
    cv_done.notify_all();
  }
  bool dropped(const Job& j) { std::lock_guard<std::mutex> lk(mu); return dropped_locked(j); }
  // (in the chunk's turn: every chunk in front of it has had its own, so this is the first stop in file order)
  void stop_at(const Job& j, uint64_t byte) { std::lock_guard<std::mutex> lk(mu); fb_seq_ = j.seq, fb_off_ = byte; }
  bool stopped(uint64_t* byte) { std::lock_guard<std::mutex> lk(mu); *byte = fb_off_; return stopped_locked(); }
  void fail(const std::string& msg)
  {
    { std::lock_guard<std::mutex> lk(mu); if (err_.empty()) err_ = msg; } // (the first error is the one reported)
    cv_done.notify_all(), cv_work.notify_all();
  }
  bool failed() { std::lock_guard<std::mutex> lk(mu); return !err_.empty(); }
  const std::string& error() const { return err_; } // (when every thread has been joined)
  bool failed_locked() const { return !err_.empty(); }
  bool stopped_locked() const { return fb_seq_ != UINT64_MAX; }

  void close(uint64_t total) // the reader: no job numbered `total` or above will come
  {
    { std::lock_guard<std::mutex> lk(mu); total_ = total; }
    cv_done.notify_all();
  }
  // the writer: the job the output is waiting for (null: the end of the input, or an error), and on to the next when it is written
  std::unique_ptr<Job> take_next()
  {
    std::unique_lock<std::mutex> lk(mu);
    cv_done.wait(lk, [&] { return finished_.count(next_seq_) || next_seq_ >= total_ || !err_.empty(); });
    auto it = finished_.find(next_seq_);
    if (!err_.empty() || it == finished_.end()) return nullptr;
    std::unique_ptr<Job> j = std::move(it->second);
    finished_.erase(it);
    return j;
  }
  void advance()
  {
    { std::lock_guard<std::mutex> lk(mu); ++next_seq_; }
    cv_done.notify_all();
  }

private:
  bool dropped_locked(const Job& j) const { return j.raw && fb_seq_ < j.seq; } // (the host reader covers the chunk's bytes)
  bool turn(std::unique_lock<std::mutex>& lk, const Job& j)
  {
    cv_done.wait(lk, [&] { return next_seq_ == j.seq || !err_.empty(); });
    return err_.empty() && !dropped_locked(j);
  }
  uint64_t next_seq_ = 0, total_ = UINT64_MAX;
  std::map<uint64_t, std::unique_ptr<Job>> finished_;
  bool seekable_ = false;
  off_t file_off_ = 0;
  uint64_t fb_seq_ = UINT64_MAX, fb_off_ = 0; // the first chunk that stopped early, and the byte the host reader starts at
  std::string err_;
};

// each read shares one unit among the references it keeps (src/query.cpp:168-170)
static void add_weights(const kr_result_view& rv, std::vector<double>& wc, double& tw)
{
  for (uint32_t r = 0; r < rv.nreads; ++r) {
    uint32_t o = rv.read_off[r], n = rv.read_cnt[r], ns = 0;
    for (uint32_t i = o; i < o + n; ++i) ns += rv.rec_sel[i];
    const double w = 1.0 / ns;
    for (uint32_t i = o; i < o + n; ++i)
      if (rv.rec_sel[i]) {
        const uint32_t se = rv.rec_key[i] >> 1;
        if (se < wc.size()) wc[se] += w;
        tw += w;
      }
  }
}

// What the threads of a run share: reader (the main thread) -> todo -> workers -> OutputOrder -> writer.
struct Run {
  const Settings& s;
  explicit Run(const Settings& s_) : s(s_) {}
  FILE* out = stdout;
  kr_host_index* hx = nullptr;
  kr_index_view view;
  kr_place_tree* ptree = nullptr;
  std::vector<kr_index*> dix;
  kr_fastx* fx = nullptr; // (opened before the workers start; they hand batches back to it)
  // --gpu-parse (plain regular files; block-gzipped ones: `bgzf` below): the reader only moves bytes into page-locked chunks cut at guessed record starts; each worker
  // finds the records of its chunks on its GPU (kr_batch_submit_fastq / kr_batch_submit_fasta with KR_TILE_DEVICE: long records are
  // tiled on the device).  The first chunk that stops early (a record that is not clean four-line FASTQ, a wrong cut, a batch that
  // overflows) names the byte where the host reader (kr_fastx_open_at) takes over for good, as the pool reader's "first surprise ->
  // sequential to the end" (kr_host.cpp).  `place`: the batch is queued with KR_TAP_ACCS and placed where it lies
  // (kr_place_stream_parsed: lengths and ids from the chunk, on the device); `seek`: queued with no flag, collected, and formatted
  // with the names cut out of the chunk.  Their rows go through the job's text and the writer, as the host reader's do.
  bool gpu_parse = false;
  int qfd = -1;
  uint64_t qsize = 0;
  bool fasta_parse = false; // a file whose first byte is '>' is cut and parsed as FASTA; any other as FASTQ
  // a block-gzipped file: the chunks are whole members, inflated on the device (kr_batch_submit_bgzf) into the job's `raw`; an early
  // stop is a BGZF virtual offset and kr_fastx_open_at_bgzf takes over there.  Every `raw` buffer has a buffer for the members.
  bool bgzf = false;
  std::map<uint8_t*, uint8_t*> comp_of;
  // --gpu-inflate, an ordinary gzip file: the reader's bytes come from the device inflater (kr_gzdev_read) in place of pread; offsets
  // are inflated offsets, and an early stop hands over through kr_fastx_open_at_gzip from the inflater's restart point (kr_gzdev_point)
  kr_gzdev* gz = nullptr;
  uint64_t chunk_cap() const { return s.chunk_bytes + (bgzf ? 2 * 65536 : 0); } // (a chunk may begin and end inside a member)

  OutputOrder order;
  // under order.mu, waited for on order.cv_work (gpu_done: cv_done)
  std::deque<std::unique_ptr<Job>> todo;
  bool eof = false;
  std::vector<uint8_t*> raw_free; // page-locked chunk buffers not in use
  uint64_t gpu_issued = 0, gpu_done = 0;
  int workers_ready = 0;
  std::vector<kr_stream*> streams_to_free;
  // --summarize: reference -> weighted read count (src/krepp.cpp:374-378), by colour id; every worker sums its batches in an array
  // of its own (264 M rows per 8 M reads on a 1000-genome index: a shared map under a mutex was the whole run) and adds it here
  // when it ends -- the reference adds per batch under `omp critical`, in whatever order the tasks finish
  std::vector<double> wcount;
  double twcount = 0;

  std::atomic<uint64_t> nreads_dev{0}; // records found on the device so far, in the output's order (advanced in a chunk's turn)
  std::atomic<uint64_t> nreads_seek{0}; // seek --gpu-seek: reads whose rows the seek kernels wrote ([timing] only)
  // seek --extract-*: the two files (the writer's, in the report's order), and for [timing] the reads, record bytes and kernel time
  FILE *ex_matched = nullptr, *ex_unmatched = nullptr;
  std::atomic<uint64_t> ex_reads{0}, ex_nmatched{0}, ex_bytes_m{0}, ex_bytes_u{0}, ex_kernel_us{0};
  // paired reads: the mates' file, their report (--output-path2) and extract files, and for [timing] the pairs
  int qfd2 = -1;
  uint64_t qsize2 = 0;
  FILE *out2 = nullptr, *ex_matched2 = nullptr, *ex_unmatched2 = nullptr;
  std::atomic<uint64_t> ex_pairs{0}, ex_pairs_matched{0}, ex_pair_bytes{0}, ex_pair_kernel_us{0};
  uint64_t nbatches = 0, nreads_total = 0; // the reader's
  // the writer's.  place --summarize: counts per placement-tree node, summed in input order; placements of a 512-read group that
  // straddles two jobs wait in `carry` (the groups are the reference's batches)
  bool jplace_prev = false;
  std::vector<double> pwcount;
  double ptwcount = 0;
  std::vector<kr_placement> carry;

  // "Loading the index and initializing..." (src/krepp.cpp:756-757) ends when the index is in device memory: t_init.  The elapsed
  // time reported at the end is everything after it -- the workers' streams and page-locked buffers, then the batch loop
  // (estimate_distances(), src/krepp.cpp:347-394,759-762: the reference's clock covers all it does after the index load, so this
  // one does too since round 6; until then it began when the streams were ready) -- taken when the last row has been written and
  // before anything is torn down, as the reference takes it before its destructors run.  The reader opens the query file and
  // parses the first batches while the streams come up.
  Clock::time_point t_init, t_loop; // t_loop: when the last worker was ready ([timing] only)
  std::atomic<uint64_t> ns_parse{0}, ns_job{0}, ns_dev{0}, ns_fmt{0}, ns_write{0};
  std::atomic<uint64_t> nb_dev_text{0}, nb_host_text{0}; // `dist` batches (pieces of them) written from device text / through kr_format_dist
  std::atomic<int> worker_ids{0};
  // --bgzf-out: the report's bytes before and after deflation, and the pieces deflated on the device / by the host encoder
  std::atomic<uint64_t> nb_plain{0}, nb_comp{0}, n_dev_deflate{0}, n_host_deflate{0};
  std::string deflated(const char* p, size_t n);
  void put(const char* p, size_t n);
  double at() const { return std::chrono::duration<double>(Clock::now() - t_init).count(); } // seconds since the query phase began

  void start_up(const Args& a);
  void open_input();
  void worker_ready(const char* err);
  std::unique_ptr<Job> next_job();
  void chunk_done(uint8_t* raw, uint8_t* raw2 = nullptr);
  void check_pair_inputs();
  void read_pairs();
  void enqueue(std::unique_ptr<Job> j);
  void read_chunks();
  void read_chunks_bgzf();
  void read_chunks_gzip();
  void chunks_done(uint64_t foreign_at);
  void read_host();
  void end_of_input();
  void write_loop();
  int finish();
};

// the output file, the index on the host and on every GPU, the placement tree, the report's first lines
void Run::start_up(const Args& a)
{
  if (s.paired()) check_pair_inputs(); // (refused before anything is loaded or created)
  if (a.has("--output-path")) {
    out = fopen(a.get("--output-path").c_str(), "w");
    if (!out) error_exit("Failed to open " + a.get("--output-path"));
  }
  if (!s.extract_matched.empty() && !(ex_matched = fopen(s.extract_matched.c_str(), "wb"))) error_exit("Failed to open " + s.extract_matched);
  if (!s.extract_unmatched.empty() && !(ex_unmatched = fopen(s.extract_unmatched.c_str(), "wb"))) error_exit("Failed to open " + s.extract_unmatched);
  if (!s.output2.empty() && !(out2 = fopen(s.output2.c_str(), "w"))) error_exit("Failed to open " + s.output2);
  if (!s.extract_matched2.empty() && !(ex_matched2 = fopen(s.extract_matched2.c_str(), "wb"))) error_exit("Failed to open " + s.extract_matched2);
  if (!s.extract_unmatched2.empty() && !(ex_unmatched2 = fopen(s.extract_unmatched2.c_str(), "wb"))) error_exit("Failed to open " + s.extract_unmatched2);
  fprintf(stderr, "Loading the index and initializing...\n");
  if (s.seek ? kr_host_sketch_load(s.index_arg.c_str(), &hx) : kr_host_index_load(s.index_arg.c_str(), &hx)) error_exit(kr_last_error());
  kr_host_index_view(hx, &view);
  if (s.place) {
    auto slurp = [](const std::string& path) {
      std::string text;
      FILE* tf = fopen(path.c_str(), "rb");
      if (!tf) error_exit("Error opening " + path);
      char buf[65536];
      size_t n;
      while ((n = fread(buf, 1, sizeof(buf), tf)) > 0) text.append(buf, n);
      fclose(tf);
      return text;
    };
    if (a.has("--lineage-file")) { // src/krepp.cpp:742-744: -l takes precedence over -t and the backbone
      if (kr_place_tree_create_lineage(hx, slurp(a.get("--lineage-file")).c_str(), &ptree)) error_exit(kr_last_error());
      fprintf(stderr, "Placing given sequences on the taxonomic lineage...\n");
    } else {
      std::string nwk_text;
      if (a.has("--nwk-file")) nwk_text = slurp(a.get("--nwk-file"));
      if (kr_place_tree_create(hx, a.has("--nwk-file") ? nwk_text.c_str() : nullptr, &ptree)) error_exit(kr_last_error());
      fprintf(stderr, "Placing given sequences on the backbone tree...\n");
    }
    view.node_kind = kr_place_tree_kinds(ptree); // leaves absent from the placement tree become null nodes
    pwcount.assign(kr_place_tree_nnodes(ptree) + 1, 0.0);
  }
  if (s.summarize && !s.place) wcount.assign((size_t)view.tree_nnodes + 2, 0.0);
  // the index crosses PCIe once; the other GPUs receive it by RCCL broadcast over xGMI (load time only)
  dix.assign(s.ngpus, nullptr);
  if (kr_index_upload(&view, s.dev0, KR_VIEW_HOST, &dix[0])) error_exit(kr_last_error());
  if (s.ngpus > 1) {
    std::vector<int> devs;
    for (int g = 1; g < s.ngpus; ++g) devs.push_back(s.dev0 + g);
    // RCCL may print a version banner on stdout when its first communicator is made; stdout is where the report rows go
    // (src/krepp.cpp:372-382).  This process is still single-threaded here (the workers start later), so pointing file
    // descriptor 1 at stderr for the duration of the call is safe -- the application's decision, not the library's.
    fflush(stdout);
    const int saved_out = dup(1);
    if (saved_out >= 0) (void)dup2(2, 1);
    const int brc = kr_index_broadcast(dix[0], s.ngpus - 1, devs.data(), dix.data() + 1);
    if (saved_out >= 0) {
      fflush(stdout);
      (void)dup2(saved_out, 1);
      close(saved_out);
    }
    if (brc) error_exit(kr_last_error());
  }
  t_init = t_loop = Clock::now();
  if (s.seek) { // QuerySketch::header_dreport (src/krepp.cpp:305-309)
    const std::string h = "# software: krepp\tversion: " KREPP_VERSION "\tinvocation :" + s.invocation + "\nSEQ_ID\tDIST\n";
    put(h.data(), h.size());
    if (out2) { // (the mates' report: the same first lines)
      const std::string c = s.bgzf_out ? deflated(h.data(), h.size()) : h;
      fwrite(c.data(), 1, c.size(), out2);
    }
  } else if (!s.place) { // header (src/krepp.cpp:311-319)
    const std::string h = "# software: krepp\tversion: " KREPP_VERSION "\tinvocation :" + s.invocation + "\n" +
                          (s.summarize ? "REFERENCE_NAME\tWEIGHTED_COUNT\tSEQUENCE_ABUNDANCE" : "SEQ_ID\tREFERENCE_NAME\tDIST") + "\n";
    put(h.data(), h.size());
  } else { // jplace opening or tabular header (src/krepp.cpp:440-447)
    char* t = nullptr;
    uint64_t l = 0;
    if (kr_place_frame(ptree, 0, s.tabular, s.invocation.c_str(), 0, &t, &l)) error_exit(kr_last_error());
    put(t, l);
    kr_free(t);
  }
  order.open(out, s.dev_text && !s.serial_write);
}

// --bgzf-out: p[0 .. n) as BGZF members, deflated by the host encoder in the calling thread (what the device's kernel would write)
std::string Run::deflated(const char* p, size_t n)
{
  std::string c((size_t)kr_bgzf_deflate_bound_member(n, s.bgzf_member), '\0');
  uint64_t len = 0;
  if (kr_bgzf_deflate_host_member((const uint8_t*)p, n, s.bgzf_level, s.bgzf_member, (uint8_t*)&c[0], c.size(), &len)) error_exit(kr_last_error());
  c.resize((size_t)len);
  if (n) nb_plain += n, nb_comp += len, ++n_host_deflate;
  return c;
}

// The one way bytes reach `out` from the threads that write in turn (start_up, the writer, finish): as they are, or as BGZF members
void Run::put(const char* p, size_t n)
{
  if (!s.bgzf_out) {
    fwrite(p, 1, n, out);
    return;
  }
  const std::string c = deflated(p, n);
  fwrite(c.data(), 1, c.size(), out);
}

// The first inflated byte of a block-gzipped file ('>': FASTA), from its first member that holds one, inflated on the host.
// False: the file does not begin with BGZF members that inflate -- the host reader's case.
static bool bgzf_first_byte(int fd, uint64_t size, uint8_t* first)
{
  std::vector<uint8_t> m(65536 + 18 + 256), u(65536);
  uint64_t off = 0;
  for (int k = 0; k < 64 && off < size; ++k) {
    const ssize_t n = pread(fd, m.data(), (size_t)std::min<uint64_t>(m.size(), size - off), (off_t)off);
    const uint32_t ms = n > 0 ? kr_bgzf_member_size(m.data(), (uint64_t)n) : 0;
    uint64_t len = 0;
    if (ms == 0 || ms > (uint64_t)n || kr_debug_bgzf_inflate_host(m.data(), ms, u.data(), u.size(), &len)) return false;
    if (len) {
      *first = u[0];
      return true;
    }
    off += ms;
  }
  return false;
}

// --gpu-parse on a plain or block-gzipped regular file: the file for pread and the page-locked chunk buffers; anything else (ordinary
// gzip, a pipe): the host reader
void Run::open_input()
{
  if (s.paired()) { // (check_pair_inputs opened the files: plain FASTQ, read by pread)
    gpu_parse = true;
    for (int q = 0; q < 2 * (2 * s.nworkers + 1); ++q) { // (a job carries two chunks: the pool doubles)
      uint8_t* b_ = (uint8_t*)kr_host_alloc(chunk_cap() + 16);
      if (!b_) error_exit("cannot allocate page-locked chunk buffers for --gpu-parse");
      raw_free.push_back(b_);
    }
    return;
  }
  if (s.gpu_parse) {
    struct stat sb;
    unsigned char mg[2] = {0, 0};
    uint8_t first = 0;
    qfd = open(s.query.c_str(), O_RDONLY);
    const bool regular = qfd >= 0 && fstat(qfd, &sb) == 0 && S_ISREG(sb.st_mode);
    const bool gz = regular && pread(qfd, mg, 2, 0) == 2 && mg[0] == 0x1f && mg[1] == 0x8b;
    if (regular && gz && bgzf_first_byte(qfd, (uint64_t)sb.st_size, &first)) {
      gpu_parse = bgzf = true;
      qsize = (uint64_t)sb.st_size;
      fasta_parse = first == '>';
    } else if (regular && gz && s.gpu_inflate) { // ordinary gzip, inflated on the first GPU (FASTA or FASTQ: read_chunks_gzip, from the first inflated byte)
      if (kr_gzdev_open(s.query.c_str(), s.dev0, s.gz_super, s.gz_sub, s.gz_ratio, 8, &this->gz)) error_exit(kr_last_error());
      gpu_parse = true;
      qsize = (uint64_t)sb.st_size;
    } else if (!regular || gz) {
      if (s.extract()) // (no host fallback: the host reader keeps neither qualities nor byte spans)
        error_exit(std::string("--extract-*: ") + (regular ? "an ordinary gzip file needs --gpu-inflate" : "not a regular file") +
                   " at input offset 0: the records must be ones the GPU record finder accepts (include/krepp_amd.h)");
      if (qfd >= 0) close(qfd);
      qfd = -1; // ordinary gzip / not a regular file: the host reader
    } else {
      gpu_parse = true;
      qsize = (uint64_t)sb.st_size;
      fasta_parse = mg[0] == '>';
    }
  }
  if (!gpu_parse && kr_fastx_open(s.query.c_str(), &fx)) error_exit(kr_last_error());
  if (gpu_parse) // one buffer per worker at work, one being filled, one waiting per worker
    for (int q = 0; q < 2 * s.nworkers + 1; ++q) {
      uint8_t* b_ = (uint8_t*)kr_host_alloc(chunk_cap() + 16);
      uint8_t* c_ = bgzf ? (uint8_t*)kr_host_alloc(chunk_cap() + 16) : nullptr;
      if (!b_ || (bgzf && !c_)) error_exit("cannot allocate page-locked chunk buffers for --gpu-parse");
      raw_free.push_back(b_);
      if (bgzf) comp_of[b_] = c_;
    }
}

// a worker has its stream, or failed to get it (err); the last one stamps t_loop
void Run::worker_ready(const char* err)
{
  if (err) order.fail(err);
  std::lock_guard<std::mutex> lk(order.mu);
  if (++workers_ready == s.nworkers) t_loop = Clock::now();
}

std::unique_ptr<Job> Run::next_job()
{
  std::unique_ptr<Job> j;
  {
    std::unique_lock<std::mutex> lk(order.mu);
    order.cv_work.wait(lk, [&] { return !todo.empty() || eof; });
    if (todo.empty()) return nullptr;
    j = std::move(todo.front());
    todo.pop_front();
  }
  order.cv_work.notify_all(); // the reader may be waiting for queue space
  return j;
}

void Run::chunk_done(uint8_t* raw, uint8_t* raw2)
{
  {
    std::lock_guard<std::mutex> lk(order.mu);
    raw_free.push_back(raw);
    if (raw2) raw_free.push_back(raw2);
    ++gpu_done;
  }
  order.cv_work.notify_all();
  order.cv_done.notify_all();
}

// the reader numbers the job and queues it; the number of batches in flight is bounded
void Run::enqueue(std::unique_ptr<Job> j)
{
  {
    std::unique_lock<std::mutex> lk(order.mu);
    j->seq = nbatches++;
    if (j->raw) ++gpu_issued;
    order.cv_work.wait(lk, [&] { return todo.size() < (size_t)(2 * s.nworkers) || order.failed_locked(); });
    todo.push_back(std::move(j));
  }
  order.cv_work.notify_all();
}

// One worker: a kr_stream of its own on GPU `g`, and the job it is running.
struct Worker {
  Run& r;
  const Settings& s;
  const int g;
  Worker(Run& r_, int g_) : r(r_), s(r_.s), g(g_) {}
  kr_stream* st = nullptr;
  kr_stream* st2 = nullptr; // paired reads: the mates' stream on the same GPU (--interleaved: none, the pairs are in st's batch)
  bool text_on = false; // the stream formats `dist` rows on the device
  bool bgzf_dev = false; // --bgzf-out: the stream deflates its device text (kr_batch_collect_text_bgzf)
  bool bgzf_place = false; // place --bgzf-out --gpu-deflate: kr_place_stream hands back members (kr_stream_place_bgzf)
  // reads per submit this worker currently trusts: halved when a submit overflows a device buffer, doubled again
  // after a run of successes -- data with hundreds of rows per read settle at a piece size instead of failing a
  // full-size submit (and every intermediate size) for every batch
  size_t piece = SIZE_MAX;
  int streak = 0;
  std::vector<double> wc; // --summarize: this worker's sums
  double tw = 0;
  std::unique_ptr<Job> j; // the job at hand; empty once its rows have taken their place in the output (OutputOrder::claim)
  std::string text;       // its rows for the writer, its placements
  std::vector<kr_placement> pls;
  std::string blob; // chunk_names
  std::vector<const char*> nptr;

  void loop();
  int run_batch(size_t lo, size_t hi);
  int run_halves(size_t lo, size_t hi);
  int run_chunk();
  int collect(kr_result_view* rv, const char** dtext, uint64_t* dlen, bool* on_device);
  int chunk_names(const uint8_t* raw, uint32_t n);
  int collect_extract();
  int extract_stop(const char* reason, uint64_t pos);
  const char* make_stream(kr_stream** out);
  int run_pair_chunk();
  int pair_stop(const std::string& reason, bool mates, uint64_t pos);
  int collect_pair_side(kr_stream* q, std::string* rows, std::string& m, std::string& u, kr_extract_view* v);
  void keep_placements(int rc, kr_placement* pp, uint64_t npp, uint64_t base);
  void emit(const char* p, size_t n, bool whole_job);
  void emit_host(const char* p, size_t n); // rows a host formatter made: through the host encoder with --bgzf-out
  void append(const char* p, size_t n);    // ... for the job's text
  int collect_device_text(const char** dtext, uint64_t* dlen) { return collect_device_text(st, dtext, dlen); }
  int collect_device_text(kr_stream* q, const char** dtext, uint64_t* dlen);
  int joins() const { return (!s.tabular && !text.empty()) ? 1 : 0; } // jplace: pieces of a job are joined by the worker, jobs by the writer (src/krepp.cpp:474-484)
  void succeeded() // (grow back after a run of successes)
  {
    if (piece != SIZE_MAX && ++streak >= 16) piece = piece > SIZE_MAX / 2 ? SIZE_MAX : piece * 2, streak = 0;
  }
};

// A stream of this worker's on its GPU with everything the run asked for enabled; the reason it could not be made, or null
const char* Worker::make_stream(kr_stream** out)
{
  kr_stream* st = nullptr; // (the one being made)
  // (four times the reads of a batch: a batch of contigs is submitted as tiles of 128 k-mer positions, include/krepp_amd.h)
  if (kr_stream_create(r.dix[g], (s.place || s.seek) ? &s.pfront : &s.p, 4 * s.max_reads, s.max_bases, s.max_records, &st)) return kr_last_error();
  if (s.dev_text) { // (and 64 bytes of id per read)
    if (kr_stream_text_enable(st, r.hx, s.text_bytes, std::max<uint64_t>(1ull << 20, (uint64_t)s.max_reads * 64)) == 0)
      text_on = true;
    else
      fprintf(stderr, "[krepp_amd] report text on the host: %s\n", kr_last_error());
  }
  if (s.gpu_seek && kr_stream_seek_enable(st, s.text_bytes, std::max<uint64_t>(1ull << 20, (uint64_t)s.max_reads * 64))) return kr_last_error();
  if (s.bgzf_out && (text_on || s.gpu_seek)) {
    if (kr_stream_bgzf_out_enable(st)) return kr_last_error();
    if (s.bgzf_level != 1 && kr_stream_bgzf_out_level(st, s.bgzf_level)) return kr_last_error();
    bgzf_dev = true;
  }
  if ((s.bgzf_out || s.extract_bgzf) && s.bgzf_member != 65280 && kr_stream_bgzf_member(st, s.bgzf_member)) return kr_last_error();
  if (s.gpu_deflate) {
    if (kr_stream_place_bgzf(st, s.bgzf_level)) return kr_last_error();
    bgzf_place = true;
  }
  if (r.gpu_parse && kr_stream_fastq_enable(st, r.chunk_cap())) return kr_last_error();
  if (r.bgzf && kr_stream_bgzf_enable(st, r.chunk_cap())) return kr_last_error();
  if (s.extract() && kr_stream_extract_enable(st, s.extract_max)) return kr_last_error();
  *out = st;
  return nullptr;
}

void Worker::loop()
{
  const int wid = r.worker_ids++;
  double t_first = -1, t_last = 0;
  uint64_t njobs = 0;
  wc.assign(r.wcount.size(), 0.0);
  if (const char* err = make_stream(&st)) return r.worker_ready(err);
  if (s.paired()) { // both streams leave the split to kr_batch_extract_pair
    if (!s.interleaved)
      if (const char* err = make_stream(&st2)) return r.worker_ready(err);
    if (kr_stream_extract_defer(st, 1) || (st2 && kr_stream_extract_defer(st2, 1))) return r.worker_ready(kr_last_error());
  }
  const double t_ready = r.at();
  r.worker_ready(nullptr);
  while ((j = r.next_job())) {
    kr_fastx_held* const held = j->held; // (what outlives a job that is handed over: the reader's buffers, the chunk's)
    uint8_t* const raw = j->raw;
    uint8_t* const raw2 = j->raw2;
    const int rc = s.paired() ? run_pair_chunk() : raw ? run_chunk() : run_batch(0, j->n);
    if (raw) r.chunk_done(raw, raw2);
    if (held) kr_fastx_release(r.fx, held); // (the batch's buffers go back to the reader)
    t_last = r.at(), ++njobs;
    if (t_first < 0) t_first = t_last;
    if (j) {
      if (rc) r.order.fail(kr_last_error()), text.clear(), pls.clear();
      r.order.finish(std::move(j), text, pls);
    }
    text.clear(), pls.clear();
  }
  if (s.timing) fprintf(stderr, "[timing] worker %d: stream ready %.3f s into the initialisation, first batch done at %.3f s, last of %llu at %.3f s\n", wid, t_ready, t_first, (unsigned long long)njobs, t_last);
  std::lock_guard<std::mutex> lk(r.order.mu);
  for (size_t q = 0; q < wc.size(); ++q) r.wcount[q] += wc[q];
  r.twcount += tw;
  r.streams_to_free.push_back(st); // (torn down with the index, after the elapsed time has been taken)
  if (st2) r.streams_to_free.push_back(st2);
}

// Rows in the job's turn: into their place in the file, or written now.
void Worker::emit(const char* p, size_t n, bool whole_job)
{
  off_t at_off = -1;
  if (!r.order.claim(j, n, whole_job, &at_off)) return;
  auto t_w = Clock::now();
  if (at_off >= 0) {
    // A batch's text is hundreds of megabytes (262,144 reads x 33 rows x 28 bytes), and one thread copies 2.5-5 GB/s into the
    // page cache: with two workers the 38 GB of a 50 M-read run were written at 5 GB/s and the run was that (round 6,
    // profiles/round6_cli_syn1000_50m.txt).  The text goes out in slices of at least 16 MB, side by side (KR_CLI_WRITE_THREADS,
    // default 4 per worker).
    const int fd = fileno(r.out);
    auto write_slice = [&](size_t a, size_t b) {
      size_t done = a;
      while (done < b) {
        const ssize_t w = pwrite(fd, p + done, b - done, at_off + (off_t)done);
        if (w < 0) {
          if (errno == EINTR) continue;
          r.order.fail(std::string("cannot write the output: ") + strerror(errno));
          break;
        }
        done += (size_t)w;
      }
    };
    const size_t nsl = std::max<size_t>(1, std::min<size_t>((size_t)s.write_threads, n >> 24));
    std::vector<std::thread> ws_;
    for (size_t q = 1; q < nsl; ++q) ws_.emplace_back(write_slice, n * q / nsl, n * (q + 1) / nsl);
    write_slice(0, n / nsl);
    for (auto& t_ : ws_) t_.join();
  } else if (n) {
    fwrite(p, 1, n, r.out);
  }
  r.ns_write += since(t_w);
}

// What a submit's rows are collected as: device text where the stream formats it (*on_device), else the row view
// (KR_ERR_UNSUPPORTED: a DIST the device does not format -- the batch's rows, for the host formatter)
int Worker::collect(kr_result_view* rv, const char** dtext, uint64_t* dlen, bool* on_device)
{
  if (!text_on) return kr_batch_collect(st, rv);
  int rc = collect_device_text(dtext, dlen);
  *on_device = rc == 0;
  if (rc == KR_ERR_UNSUPPORTED) rc = kr_batch_collect(st, rv);
  return rc;
}

// The batch's device text: the bytes the output takes -- plain, or deflated into BGZF members where they lie (--bgzf-out)
int Worker::collect_device_text(kr_stream* q, const char** dtext, uint64_t* dlen)
{
  if (!bgzf_dev) return kr_batch_collect_text(q, dtext, dlen);
  const uint8_t* comp = nullptr;
  uint64_t text_len = 0;
  const int rc = kr_batch_collect_text_bgzf(q, &comp, dlen, &text_len);
  *dtext = (const char*)comp;
  if (!rc && text_len) r.nb_plain += text_len, r.nb_comp += *dlen, ++r.n_dev_deflate;
  return rc;
}

void Worker::emit_host(const char* p, size_t n)
{
  if (!s.bgzf_out) return emit(p, n, false);
  const std::string c = r.deflated(p, n);
  emit(c.data(), c.size(), false);
}

void Worker::append(const char* p, size_t n)
{
  if (bgzf_place) { // members already (kr_stream_place_bgzf): what they inflate to is in their trailers
    uint32_t nm = 0;
    uint64_t cb = 0, ub = 0;
    if (n && kr_bgzf_walk((const uint8_t*)p, n, UINT64_MAX, &nm, &cb, &ub) == 0) r.nb_plain += ub, r.nb_comp += n;
    text.append(p, n);
  } else if (s.bgzf_out) text += r.deflated(p, n);
  else text.append(p, n);
}

// place --summarize: the piece's placements, `read` counted from `base`
void Worker::keep_placements(int rc, kr_placement* pp, uint64_t npp, uint64_t base)
{
  for (uint64_t i = 0; !rc && i < npp; ++i) {
    pp[i].read = (uint32_t)(base + pp[i].read);
    pls.push_back(pp[i]);
  }
  kr_free(pp);
}

int Worker::run_halves(size_t lo, size_t hi)
{
  const size_t mid = lo + (hi - lo) / 2;
  const int rc = run_batch(lo, mid);
  return rc ? rc : run_batch(mid, hi);
}

// reads [lo, hi) of a host job; a batch that overflows a device-side buffer (KR_ERR_CAPACITY: unusually many
// table hits or records per read) is resubmitted in halves, as include/krepp_amd.h prescribes
int Worker::run_batch(size_t lo, size_t hi)
{
  const size_t n = hi - lo;
  if (n > piece && n > 1) return run_halves(lo, hi); // known to be too much for one submit
  const bool whole_job = lo == 0 && hi == j->n;
  const char* const* nm = j->names + lo;
  std::vector<uint64_t> offs(n + 1);
  for (size_t i = lo; i <= hi; ++i) offs[i - lo] = j->offsets[i] - j->offsets[lo];
  kr_result_view rv;
  char* txt = nullptr;
  uint64_t len = 0, dlen = 0;
  const char* dtext = nullptr;
  bool on_device = false;
  auto t_dev = Clock::now();
  int rc;
  if (s.gpu_seek) { // the seek kernels: the report comes back as bytes, in the job's text for the writer
    std::vector<uint32_t> id_off(n + 1);
    for (size_t i = 0; i < n; ++i) id_off[i] = (uint32_t)(nm[i] - j->blob);
    id_off[n] = hi < j->n ? (uint32_t)(nm[n] - j->blob) : (uint32_t)j->blob_bytes;
    rc = kr_batch_submit_text(st, j->bases + j->offsets[lo], offs.data(), (uint32_t)n, KR_BASES_HOST | KR_SEEK, j->blob, id_off.data(), 1);
    if (!rc) rc = collect_device_text(&dtext, &dlen);
    r.ns_dev += since(t_dev);
    if (rc == KR_ERR_CAPACITY && n > 1) {
      piece = std::min(piece, (n + 1) / 2);
      streak = 0;
      return run_halves(lo, hi);
    }
    if (rc) return rc;
    text.append(dtext, dlen); // (members, with --bgzf-out: they concatenate as their texts do)
    r.nreads_seek += n;
    succeeded();
    return 0;
  }
  if (text_on) {
    std::vector<uint32_t> id_off(n + 1);
    for (size_t i = 0; i < n; ++i) id_off[i] = (uint32_t)(nm[i] - j->blob);
    id_off[n] = hi < j->n ? (uint32_t)(nm[n] - j->blob) : (uint32_t)j->blob_bytes;
    rc = kr_batch_submit_text(st, j->bases + j->offsets[lo], offs.data(), (uint32_t)n, KR_BASES_HOST | s.rows_flags(true), j->blob, id_off.data(), 1);
  } else {
    rc = kr_batch_submit(st, j->bases + j->offsets[lo], offs.data(), (uint32_t)n, KR_BASES_HOST | s.rows_flags(false));
  }
  if (!rc) rc = s.place ? kr_batch_wait(st) : collect(&rv, &dtext, &dlen, &on_device); // place: the records stay on the device
  r.ns_dev += since(t_dev);
  auto t_fmt = Clock::now();
  if (rc == KR_ERR_CAPACITY && n > 1) {
    piece = std::min(piece, (n + 1) / 2);
    streak = 0;
    return run_halves(lo, hi);
  }
  if (!rc && s.seek) rc = kr_format_seek(r.hx, r.dix[g], &rv, s.p.hdist_th, nm, &txt, &len);
  if (!rc && on_device) {
    ++r.nb_dev_text;
    emit(dtext, dlen, whole_job); // (`j` is gone if these were all its rows)
    succeeded();
    return 0;
  }
  if (!rc && s.plain_dist()) {
    rc = kr_format_dist(r.hx, &rv, nm, &txt, &len);
    if (!rc) ++r.nb_host_text;
  }
  if (!rc && s.summarize && !s.place) add_weights(rv, wc, tw);
  if (!rc && s.place) {
    int prev = joins();
    kr_placement* pp = nullptr;
    uint64_t npp = 0;
    rc = kr_place_stream(r.hx, r.dix[g], r.ptree, st, (uint32_t)n, offs.data(), nm, &s.p, s.tabular, &prev, &txt, &len, s.tabular == 2 ? &pp : nullptr,
                         s.tabular == 2 ? &npp : nullptr);
    keep_placements(rc, pp, npp, j->first_read + lo);
  }
  if (!rc && txt && s.dev_text)
    emit_host(txt, len); // (in order with the pieces the device wrote)
  else if (!rc && txt)
    append(txt, len);
  kr_free(txt);
  r.ns_fmt += since(t_fmt);
  if (!rc) succeeded();
  return rc;
}

// the accepted records' names, NUL-terminated, cut out of the chunk for the host formatters
int Worker::chunk_names(const uint8_t* raw, uint32_t n)
{
  const uint64_t* np = nullptr;
  const uint32_t* nl = nullptr;
  const int rc = kr_batch_fastq_names(st, &np, &nl);
  if (rc) return rc;
  std::vector<size_t> at_(n);
  blob.clear();
  for (uint32_t i = 0; i < n; ++i) at_[i] = blob.size(), blob.append((const char*)raw + np[i], nl[i]), blob.push_back('\0');
  nptr.resize(n);
  for (uint32_t i = 0; i < n; ++i) nptr[i] = blob.data() + at_[i];
  return 0;
}

// --gpu-parse: the chunk's records found on the device, submitted again from `consumed` while a batch stops at capacity; anything
// else that keeps it from being taken whole (`fell`) hands the file to the host reader from the first record not taken
int Worker::run_chunk()
{
  if (r.order.dropped(*j)) return 0;
  uint64_t pos = 0, nr_job = 0;
  std::vector<double> wc_job(wc.size(), 0.0); // (sums that count only once the chunk's turn confirms it was not dropped)
  double tw_job = 0;
  bool fell = false;
  // (KR_TILE_DEVICE: a long record stays with the device, tiled there)
  // (--gpu-seek: long records too, split by the seek units)
  const uint32_t flags = s.gpu_seek ? (KR_SEEK | KR_TILE_DEVICE) : s.rows_flags(text_on) | (s.seek ? 0u : KR_TILE_DEVICE);
  while (pos < j->raw_len) {
    const uint8_t* raw = j->raw + pos;
    kr_fastq_parse fp;
    auto t_dev = Clock::now();
    int rc;
    if (j->comp && pos == 0) { // (after KR_FASTQ_CAPACITY the chunk's bytes are in `raw`: the submits below)
      rc = kr_batch_submit_bgzf(st, j->comp, j->comp_len, j->skip, j->raw_len, j->raw, flags, j->fasta ? 1u : 0u, (j->fasta ? j->closed : j->at_eof) ? 1u : 0u, &fp);
      if (rc == KR_ERR_FORMAT) // as the host reader reports a member that does not inflate: the file, and where
        r.order.fail("damaged block-gzipped file: " + s.query + ": in the members from offset " + std::to_string(j->m_off[0]) + ": " + kr_last_error());
    } else
      rc = j->fasta ? kr_batch_submit_fasta(st, raw, j->raw_len - pos, flags, j->closed ? 1u : 0u, &fp)
                    : kr_batch_submit_fastq(st, raw, j->raw_len - pos, flags, j->at_eof ? 1u : 0u, &fp);
    if (rc) return rc;
    if (fp.nreads) {
      kr_result_view rv;
      char* txt = nullptr;
      uint64_t len = 0, dlen = 0;
      const char* dtext = nullptr;
      bool on_device = false;
      if (s.gpu_seek)
        rc = collect_device_text(&dtext, &dlen);
      else if (!s.place)
        rc = collect(&rv, &dtext, &dlen, &on_device); // (place: kr_place_stream_parsed waits for the batch)
      r.ns_dev += since(t_dev);
      auto t_fmt = Clock::now();
      if (s.gpu_seek) {
        if (!rc) text.append(dtext, dlen);
        if (!rc && s.extract()) rc = collect_extract();
      } else if (!rc && on_device) {
        ++r.nb_dev_text;
        emit(dtext, dlen, false);
      } else if (!rc && s.summarize && !s.place) {
        add_weights(rv, wc_job, tw_job);
      } else if (!rc && !s.place) {
        rc = chunk_names(raw, fp.nreads);
        if (!rc) rc = s.seek ? kr_format_seek(r.hx, r.dix[g], &rv, s.p.hdist_th, nptr.data(), &txt, &len) : kr_format_dist(r.hx, &rv, nptr.data(), &txt, &len);
        if (!rc && !s.seek) ++r.nb_host_text;
      } else if (!rc) {
        int prev = joins();
        kr_placement* pp = nullptr;
        uint64_t npp = 0;
        rc = kr_place_stream_parsed(r.hx, r.dix[g], r.ptree, st, raw, &s.p, s.tabular, &prev, &txt, &len, s.tabular == 2 ? &pp : nullptr,
                                    s.tabular == 2 ? &npp : nullptr);
        keep_placements(rc, pp, npp, nr_job); // (`read`: the number within the chunk; the chunk's first read is known when its turn comes)
      }
      if (!rc && txt && s.plain_dist())
        emit_host(txt, len);
      else if (!rc && txt)
        append(txt, len);
      kr_free(txt);
      r.ns_fmt += since(t_fmt);
      if (rc == KR_ERR_CAPACITY) { // more records or text than a batch holds: the host reader takes over at this batch's first record
        if (s.extract()) return extract_stop("more report text than a batch holds", pos);
        fell = true;
        break;
      }
      if (rc) return rc;
      nr_job += fp.nreads;
    }
    pos += fp.consumed;
    if (fp.status == KR_FASTQ_OK) break;
    if (fp.status == KR_FASTQ_CAPACITY && fp.nreads) continue;
    if (s.extract()) // (no host fallback: nothing is silently left out of either file)
      return extract_stop(fp.status == KR_FASTQ_NOT_CLEAN ? "a record that is not clean (CRLF in a FASTQ, a stray '>' '+' '@', a quality line of another length)"
                          : fp.status == KR_FASTQ_INCOMPLETE ? "an incomplete record (cut short, or a last line without '\\n')"
                                                             : "a record that does not fit a batch",
                          pos);
    fell = true; // not clean, a record cut by the end of the chunk or the file: the host reader from here
    break;
  }
  // in the output's order: only a chunk that no earlier chunk's stop has dropped counts
  if (!r.order.wait_turn(*j)) {
    text.clear(), pls.clear(); // (`place` / `seek`: rows made before the earlier chunk's stop was known)
    j->ex_matched.clear(), j->ex_unmatched.clear();
    return 0;
  }
  for (size_t q = 0; q < wc_job.size(); ++q) wc[q] += wc_job[q];
  tw += tw_job;
  // place --summarize sums per 512 reads by global read number: every chunk in front of this one has had its turn
  j->first_read = r.nreads_dev, j->n = (size_t)nr_job;
  for (kr_placement& x : pls) x.read = (uint32_t)(j->first_read + x.read);
  r.nreads_dev += nr_job;
  if (s.gpu_seek) r.nreads_seek += nr_job;
  if (fell) r.order.stop_at(*j, j->comp ? j->voffset(pos) : j->raw_off + pos);
  return 0;
}

// seek --extract-*: the parts of the batch just collected, appended to the job's two byte strings (plain, or as BGZF members)
int Worker::collect_extract()
{
  kr_extract_view v;
  const int rc = s.extract_bgzf ? kr_batch_collect_extract_bgzf(st, s.extract_which(), s.bgzf_level, &v) : kr_batch_collect_extract(st, s.extract_which(), &v);
  if (rc) return rc;
  if (v.matched) j->ex_matched.append((const char*)v.matched, (size_t)v.matched_len);
  if (v.unmatched) j->ex_unmatched.append((const char*)v.unmatched, (size_t)v.unmatched_len);
  r.ex_reads += v.nreads, r.ex_nmatched += v.nmatched, r.ex_bytes_m += v.matched_bytes, r.ex_bytes_u += v.unmatched_bytes;
  float ms = 0;
  if (s.timing && kr_debug_extract_ms(st, &ms) == 0) r.ex_kernel_us += (uint64_t)(ms * 1000.0f);
  return 0;
}

// seek --extract-*: a chunk the device cannot take whole ends the run (the host reader keeps neither qualities nor byte spans)
int Worker::extract_stop(const char* reason, uint64_t pos)
{
  // N is a byte of the file where it can be: a plain file's offset; for a block-gzipped chunk the file offset of the BGZF member that
  // holds the record's first byte, with the inflated byte inside it named beside the reason (together the virtual offset the host
  // reader is handed at such a stop); for ordinary gzip (--gpu-inflate) only the inflated offset exists
  std::string why = reason;
  uint64_t at = j->raw_off + pos;
  if (j->comp) {
    const uint64_t v = j->voffset(pos);
    at = v >> 16, why += " (inflated byte " + std::to_string(v & 0xFFFFu) + " of the BGZF member)";
  } else if (r.gz)
    why += " (offset in the inflated stream)";
  r.order.fail("--extract-*: " + why + " at input offset " + std::to_string(at) +
               ": the records must be ones the GPU record finder accepts (include/krepp_amd.h)");
  return KR_ERR_FORMAT;
}

// paired reads: a chunk the device cannot take whole ends the run, naming the file (mates: --query2's) and the byte
int Worker::pair_stop(const std::string& reason, bool mates, uint64_t pos)
{
  r.order.fail("--extract-*: " + reason + " at input offset " + std::to_string((mates ? j->raw2_off : j->raw_off) + pos) + " of " + (mates ? s.query2 : s.query) +
               ": the records must be ones the GPU record finder accepts (include/krepp_amd.h)");
  return KR_ERR_FORMAT;
}

// paired reads: one stream's rows (rows == nullptr: not asked for) and its two parts behind the pair call
int Worker::collect_pair_side(kr_stream* q, std::string* rows, std::string& m, std::string& u, kr_extract_view* v)
{
  if (rows) {
    const char* dtext = nullptr;
    uint64_t dlen = 0;
    if (int rc = collect_device_text(q, &dtext, &dlen)) return rc;
    rows->append(dtext, dlen);
  }
  const int rc = s.extract_bgzf ? kr_batch_collect_extract_bgzf(q, s.extract_which(), s.bgzf_level, v) : kr_batch_collect_extract(q, s.extract_which(), v);
  if (rc) return rc;
  if (v->matched) m.append((const char*)v->matched, (size_t)v->matched_len);
  if (v->unmatched) u.append((const char*)v->unmatched, (size_t)v->unmatched_len);
  return 0;
}

// paired reads (--query2 / --interleaved): the job's two chunks hold the same records (kr_fastq_pair_cut).  Each goes to its own
// stream, kr_batch_extract_pair splits both by the pair's verdict, and both reports and all parts are collected.  A batch that stops
// at capacity on one side leaves the two accepted prefixes of different lengths: the longer chunk is submitted once more, cut at the
// start of the first record the other side did not take, and the loop goes on behind both prefixes.  Every other stop ends the run.
int Worker::run_pair_chunk()
{
  const bool inter = s.interleaved;
  const uint32_t flags = KR_SEEK | KR_TILE_DEVICE;
  uint64_t pos[2] = {0, 0}, nr_job = 0;
  kr_stream* const q[2] = {st, st2};
  const uint8_t* const raw[2] = {j->raw, j->raw2};
  const uint64_t len[2] = {j->raw_len, j->raw2_len};
  const bool eof[2] = {j->at_eof, j->at_eof2};
  const int nside = inter ? 1 : 2;
  auto stop_reason = [](const kr_fastq_parse& fp) -> const char* {
    if (fp.status == KR_FASTQ_OK || (fp.status == KR_FASTQ_CAPACITY && fp.nreads)) return nullptr;
    return fp.status == KR_FASTQ_NOT_CLEAN ? "a record that is not clean (CRLF in a FASTQ, a stray '>' '+' '@', a quality line of another length)"
           : fp.status == KR_FASTQ_INCOMPLETE ? "an incomplete record (cut short, or a last line without '\\n')"
                                               : "a record that does not fit a batch";
  };
  while (pos[0] < len[0]) {
    if (!inter && pos[1] >= len[1]) return pair_stop("mates out of step: the mates' chunk ends in front of this record", false, pos[0]);
    kr_fastq_parse fp[2];
    auto t_dev = Clock::now();
    for (int k = 0; k < nside; ++k) {
      if (int rc = kr_batch_submit_fastq(q[k], raw[k] + pos[k], len[k] - pos[k], flags, eof[k] ? 1u : 0u, &fp[k])) return rc;
      if (const char* why = stop_reason(fp[k])) return pair_stop(why, k == 1, pos[k] + fp[k].consumed);
    }
    // the pairs both sides took: the shorter prefix (one file: an even number of records)
    const uint32_t n = inter ? fp[0].nreads & ~1u : std::min(fp[0].nreads, fp[1].nreads);
    if (n == 0) return pair_stop("a pair that does not fit a batch", false, pos[0]);
    for (int k = 0; k < nside; ++k) {
      if (fp[k].nreads == n) continue;
      const uint64_t* np = nullptr;
      const uint32_t* nl = nullptr;
      if (int rc = kr_batch_fastq_names(q[k], &np, &nl)) return rc;
      const uint64_t cut = np[n] - 1; // (the '@' of the first record the other side did not take)
      if (int rc = kr_batch_submit_fastq(q[k], raw[k] + pos[k], cut, flags, 0u, &fp[k])) return rc;
      if (fp[k].status != KR_FASTQ_OK || fp[k].nreads != n) return pair_stop("mates out of step: the two files' records do not pair up", k == 1, pos[k]);
    }
    if (int rc = kr_batch_extract_pair(st, inter ? st : st2, s.pair_rule)) return rc;
    kr_extract_view v[2];
    int rc = collect_pair_side(st, &text, j->ex_matched, j->ex_unmatched, &v[0]);
    if (!rc && !inter) rc = collect_pair_side(st2, r.out2 ? &j->text2 : nullptr, j->ex_matched2, j->ex_unmatched2, &v[1]);
    r.ns_dev += since(t_dev);
    if (rc == KR_ERR_CAPACITY) return pair_stop("more report text than a batch holds", false, pos[0]);
    if (rc) return rc;
    if (!inter && (v[0].nmatched != v[1].nmatched || v[0].nreads != v[1].nreads)) {
      r.order.fail("--extract-*: the two parts of a pair batch differ in their record counts");
      return KR_ERR_FORMAT;
    }
    const uint64_t div = inter ? 2 : 1;
    r.ex_pairs += v[0].nreads / div, r.ex_pairs_matched += v[0].nmatched / div;
    for (int k = 0; k < nside; ++k) {
      r.ex_reads += v[k].nreads, r.ex_nmatched += v[k].nmatched, r.ex_bytes_m += v[k].matched_bytes, r.ex_bytes_u += v[k].unmatched_bytes;
      r.ex_pair_bytes += v[k].matched_bytes + v[k].unmatched_bytes;
      pos[k] += fp[k].consumed;
      nr_job += fp[k].nreads;
    }
    float ms = 0;
    if (s.timing && kr_debug_extract_ms(st, &ms) == 0) r.ex_kernel_us += (uint64_t)(ms * 1000.0f), r.ex_pair_kernel_us += (uint64_t)(ms * 1000.0f);
  }
  if (!inter && pos[1] < len[1]) return pair_stop("mates out of step: this record has no mate in the first file's chunk", true, pos[1]);
  if (!r.order.wait_turn(*j)) {
    text.clear();
    j->text2.clear(), j->ex_matched.clear(), j->ex_unmatched.clear(), j->ex_matched2.clear(), j->ex_unmatched2.clear();
    return 0;
  }
  j->first_read = r.nreads_dev, j->n = (size_t)nr_job;
  r.nreads_dev += nr_job, r.nreads_seek += nr_job;
  return 0;
}

// the writer thread: the jobs' texts in input order (jobs whose rows a worker wrote pass through empty)
void Run::write_loop()
{
  while (std::unique_ptr<Job> j = order.take_next()) {
    if (s.tabular == 2) {
      const uint32_t end_group = (uint32_t)(j->first_read + j->n) >> 9;
      carry.insert(carry.end(), j->pls.begin(), j->pls.end());
      size_t cut = j->n ? carry.size() : 0; // (--gpu-parse: a chunk that was dropped, or stopped at its first record, has no reads and no last group)
      if ((j->first_read + j->n) & 511u)
        while (cut > 0 && (carry[cut - 1].read >> 9) == end_group) --cut;
      if (kr_place_summary_add(ptree, carry.data(), cut, pwcount.data(), &ptwcount)) return order.fail(kr_last_error());
      carry.erase(carry.begin(), carry.begin() + cut);
    } else if (s.place && !s.tabular) {
      if (!j->text.empty()) {
        if (jplace_prev) put(",\n", 2);
        fwrite(j->text.data(), 1, j->text.size(), out);
        jplace_prev = true;
      }
    } else {
      auto t_w = Clock::now();
      fwrite(j->text.data(), 1, j->text.size(), out);
      if (ex_matched) fwrite(j->ex_matched.data(), 1, j->ex_matched.size(), ex_matched);
      if (ex_unmatched) fwrite(j->ex_unmatched.data(), 1, j->ex_unmatched.size(), ex_unmatched);
      if (out2) fwrite(j->text2.data(), 1, j->text2.size(), out2);
      if (ex_matched2) fwrite(j->ex_matched2.data(), 1, j->ex_matched2.size(), ex_matched2);
      if (ex_unmatched2) fwrite(j->ex_unmatched2.data(), 1, j->ex_unmatched2.size(), ex_unmatched2);
      ns_write += since(t_w);
    }
    j.reset();
    order.advance();
  }
}

// --gpu-parse: the reader moves bytes only, until the file ends or a chunk stops early
void Run::read_chunks()
{
  auto t_parse = Clock::now();
  uint64_t off = 0;
  while (off < qsize) {
    uint8_t* buf = nullptr;
    {
      std::unique_lock<std::mutex> lk(order.mu);
      order.cv_work.wait(lk, [&] { return !raw_free.empty() || order.stopped_locked() || order.failed_locked(); });
      if (order.stopped_locked() || order.failed_locked()) break; // (an early stop: nothing behind it will be used)
      buf = raw_free.back();
      raw_free.pop_back();
    }
    const uint64_t want = std::min<uint64_t>(s.chunk_bytes, qsize - off);
    uint64_t got = 0;
    while (got < want) {
      const ssize_t k = pread(qfd, buf + got, want - got, (off_t)(off + got));
      if (k <= 0) error_exit("cannot read " + s.query);
      got += (uint64_t)k;
    }
    // The chunk ends at its last record start: what lies in front of it is whole records.  None (FASTA: the chunk's one record is
    // longer than the chunk; FASTQ: no line that looks like a record start): it goes out whole, its last record stops INCOMPLETE
    // and the host reader takes over there
    const bool last = off + want >= qsize;
    const uint64_t c = last ? 0 : fasta_parse ? kr_fasta_chunk_cut(buf, want) : kr_fastq_chunk_cut(buf, want);
    const uint64_t cut = c ? c : want;
    std::unique_ptr<Job> j(new Job());
    j->raw = buf, j->raw_len = cut, j->raw_off = off, j->at_eof = last && cut == want;
    j->fasta = fasta_parse, j->closed = last || (fasta_parse && c);
    off += cut;
    enqueue(std::move(j));
  }
  ns_parse += since(t_parse);
  chunks_done(UINT64_MAX);
}

// paired reads: both files must be plain FASTQ (gzip, BGZF and FASTA pairs are not built); settled before anything is loaded
void Run::check_pair_inputs()
{
  auto open_plain = [&](const std::string& path, int* fd, uint64_t* size) {
    struct stat sb;
    unsigned char mg[2] = {0, 0};
    *fd = open(path.c_str(), O_RDONLY);
    if (*fd < 0) error_exit("Failed to open the file at " + path);
    if (fstat(*fd, &sb) != 0 || !S_ISREG(sb.st_mode)) error_exit("paired reads: not a regular file: " + path);
    *size = (uint64_t)sb.st_size;
    const ssize_t k = pread(*fd, mg, 2, 0);
    if (k == 2 && mg[0] == 0x1f && mg[1] == 0x8b)
      error_exit("paired reads: only plain FASTQ files are accepted so far, not gzip or BGZF (with or without --gpu-inflate): " + path);
    if (k >= 1 && mg[0] != '@') error_exit(std::string("paired reads: only plain FASTQ files are accepted so far, not ") + (mg[0] == '>' ? "FASTA" : "this file") + ": " + path);
  };
  open_plain(s.query, &qfd, &qsize);
  if (!s.interleaved) open_plain(s.query2, &qfd2, &qsize2);
}

// paired reads: both files by pread in chunks, cut behind the same number of whole records (kr_fastq_pair_cut counts newlines);
// each offset advances by its own cut.  --interleaved: one file, cut behind an even number of records
void Run::read_pairs()
{
  auto t_parse = Clock::now();
  const bool inter = s.interleaved;
  uint64_t off[2] = {0, 0};
  const uint64_t size[2] = {qsize, inter ? 0 : qsize2};
  const int fd[2] = {qfd, qfd2};
  const int nside = inter ? 1 : 2;
  auto uneven = [&] {
    order.fail(inter ? "--interleaved: " + s.query + " (offset " + std::to_string(off[0]) + "): the mates do not hold the same number of records -- an odd or incomplete record is left"
                     : "paired reads: " + s.query + " (offset " + std::to_string(off[0]) + ") and " + s.query2 + " (offset " + std::to_string(off[1]) +
                         ") do not hold the same number of records");
  };
  while (off[0] < size[0] || off[1] < size[1]) {
    if (!inter && (off[0] >= size[0] || off[1] >= size[1])) { // bytes left in one file only
      uneven();
      break;
    }
    uint8_t* buf[2] = {nullptr, nullptr};
    {
      std::unique_lock<std::mutex> lk(order.mu);
      order.cv_work.wait(lk, [&] { return raw_free.size() >= (size_t)nside || order.failed_locked(); });
      if (order.failed_locked()) break;
      for (int k = 0; k < nside; ++k) buf[k] = raw_free.back(), raw_free.pop_back();
    }
    uint64_t want[2] = {0, 0};
    bool read_ok = true;
    for (int k = 0; k < nside && read_ok; ++k) {
      want[k] = std::min<uint64_t>(s.chunk_bytes, size[k] - off[k]);
      uint64_t got = 0;
      while (got < want[k]) {
        const ssize_t n = pread(fd[k], buf[k] + got, want[k] - got, (off_t)(off[k] + got));
        if (n <= 0) {
          order.fail("cannot read " + (k ? s.query2 : s.query));
          read_ok = false;
          break;
        }
        got += (uint64_t)n;
      }
    }
    uint64_t cut[2] = {0, 0};
    uint32_t n = 0;
    if (read_ok && kr_fastq_pair_cut(buf[0], want[0], inter ? nullptr : buf[1], want[1], s.max_reads, &cut[0], &cut[1], &n)) order.fail(kr_last_error()), read_ok = false;
    if (read_ok && n == 0) {
      const bool end0 = off[0] + want[0] >= size[0], end1 = inter || off[1] + want[1] >= size[1];
      if (end0 || end1)
        uneven(); // (what is left of a file is no whole record, or no whole pair)
      else
        order.fail("paired reads: a record longer than a chunk (" + std::to_string(s.chunk_bytes) + " bytes) at offset " + std::to_string(off[0]) + " of " + s.query + " or offset " +
                   std::to_string(off[1]) + " of " + s.query2);
      read_ok = false;
    }
    if (!read_ok) {
      std::lock_guard<std::mutex> lk(order.mu);
      for (int k = 0; k < nside; ++k) raw_free.push_back(buf[k]);
      break;
    }
    std::unique_ptr<Job> j(new Job());
    j->raw = buf[0], j->raw_len = cut[0], j->raw_off = off[0], j->at_eof = off[0] + cut[0] >= size[0];
    if (!inter) j->raw2 = buf[1], j->raw2_len = cut[1], j->raw2_off = off[1], j->at_eof2 = off[1] + cut[1] >= size[1];
    off[0] += cut[0], off[1] += cut[1];
    enqueue(std::move(j));
  }
  ns_parse += since(t_parse);
  {
    std::unique_lock<std::mutex> lk(order.mu);
    order.cv_done.wait(lk, [&] { return gpu_done == gpu_issued || order.failed_locked(); });
  }
  close(qfd);
  if (qfd2 >= 0) close(qfd2);
  nreads_total = nreads_dev;
}

// --gpu-parse --gpu-inflate on an ordinary gzip file: read_chunks with kr_gzdev_read in place of pread.  The bytes behind a chunk's cut
// are carried to the front of the next chunk's buffer; raw_off is an inflated offset.
void Run::read_chunks_gzip()
{
  auto t_parse = Clock::now();
  std::vector<uint8_t> carry_bytes;
  uint64_t off = 0; // inflated offset of the next chunk's first byte
  bool at_end = false, first = true;
  while (!at_end) {
    uint8_t* buf = nullptr;
    {
      std::unique_lock<std::mutex> lk(order.mu);
      order.cv_work.wait(lk, [&] { return !raw_free.empty() || order.stopped_locked() || order.failed_locked(); });
      if (order.stopped_locked() || order.failed_locked()) break; // (an early stop: nothing behind it will be used)
      buf = raw_free.back();
      raw_free.pop_back();
    }
    uint64_t got = carry_bytes.size();
    if (got) memcpy(buf, carry_bytes.data(), got);
    carry_bytes.clear();
    while (got < s.chunk_bytes) {
      uint64_t k = 0;
      if (kr_gzdev_read(gz, buf + got, s.chunk_bytes - got, &k)) { // damage (the inflater hands out what lies in front of it first): the run fails here, with the chunk being filled
        order.fail(kr_last_error());
        at_end = true;
        break;
      }
      if (k == 0) {
        at_end = true;
        break;
      }
      got += k;
    }
    if (order.failed() || got == 0) { // (the buffer goes back unused)
      std::lock_guard<std::mutex> lk(order.mu);
      raw_free.push_back(buf);
      break;
    }
    if (first) fasta_parse = buf[0] == '>', first = false;
    const uint64_t c = at_end ? 0 : fasta_parse ? kr_fasta_chunk_cut(buf, got) : kr_fastq_chunk_cut(buf, got);
    const uint64_t cut = c ? c : got;
    carry_bytes.assign(buf + cut, buf + got);
    std::unique_ptr<Job> j(new Job());
    j->raw = buf, j->raw_len = cut, j->raw_off = off, j->at_eof = at_end && cut == got;
    j->fasta = fasta_parse, j->closed = at_end || (fasta_parse && c);
    off += cut;
    enqueue(std::move(j));
  }
  ns_parse += since(t_parse);
  chunks_done(UINT64_MAX);
}

// Every chunk handed out is done (an earlier one may still stop early): then the first stop, if any, is final, and the host reader
// takes over there.  foreign_at: where a block-gzipped file goes on with bytes that are no BGZF member (UINT64_MAX: nowhere) -- the
// host reader's from that offset when no chunk stopped in front of it.
void Run::chunks_done(uint64_t foreign_at)
{
  {
    std::unique_lock<std::mutex> lk(order.mu);
    order.cv_done.wait(lk, [&] { return gpu_done == gpu_issued || order.failed_locked(); });
  }
  close(qfd);
  nreads_total = nreads_dev; // (the host reader, if it takes over, numbers its reads behind the device's: place --summarize)
  uint64_t fb_off = 0;
  const bool stopped = order.stopped(&fb_off);
  if (order.failed()) return;
  if (stopped && gz) { // zlib primed at the inflater's restart point in front of the stop (none kept that far back: from the file's start)
    std::unique_ptr<kr_gzip_point> pt(new kr_gzip_point());
    const bool have = kr_gzdev_point(gz, fb_off, pt.get()) == 0;
    if (kr_fastx_open_at_gzip(s.query.c_str(), fb_off, have ? pt.get() : nullptr, &fx)) error_exit(kr_last_error());
    return;
  }
  if (stopped && (bgzf ? kr_fastx_open_at_bgzf(s.query.c_str(), fb_off >> 16, (uint32_t)(fb_off & 0xFFFFu), &fx) : kr_fastx_open_at(s.query.c_str(), fb_off, &fx)))
    error_exit(kr_last_error());
  if (!stopped && foreign_at != UINT64_MAX && kr_fastx_open_at_bgzf(s.query.c_str(), foreign_at, 0, &fx)) error_exit(kr_last_error());
}

// --gpu-parse on a block-gzipped file: the reader moves whole members, as many as inflate to a chunk, and cuts the chunk at its last
// record start (kr_bgzf_chunk_cut inflates the last members to find it); the next chunk begins at the member that holds the cut,
// `skip` bytes into it.  The device inflates the members and finds the records (kr_batch_submit_bgzf).
void Run::read_chunks_bgzf()
{
  auto t_parse = Clock::now();
  uint64_t off = 0, foreign_at = UINT64_MAX;
  uint32_t skip = 0;
  while (off < qsize) {
    uint8_t* buf = nullptr;
    {
      std::unique_lock<std::mutex> lk(order.mu);
      order.cv_work.wait(lk, [&] { return !raw_free.empty() || order.stopped_locked() || order.failed_locked(); });
      if (order.stopped_locked() || order.failed_locked()) break; // (an early stop: nothing behind it will be used)
      buf = raw_free.back();
      raw_free.pop_back();
    }
    auto give_back = [&] {
      std::lock_guard<std::mutex> lk(order.mu);
      raw_free.push_back(buf);
    };
    uint8_t* comp = comp_of[buf];
    const uint64_t want = std::min<uint64_t>(chunk_cap(), qsize - off);
    uint64_t got = 0;
    while (got < want) {
      const ssize_t k = pread(qfd, comp + got, want - got, (off_t)(off + got));
      if (k <= 0) error_exit("cannot read " + s.query);
      got += (uint64_t)k;
    }
    uint32_t nm = 0;
    uint64_t cb = 0, U = 0;
    if (kr_bgzf_walk(comp, want, s.chunk_bytes + skip, &nm, &cb, &U)) error_exit(kr_last_error());
    if (nm == 0) { // no whole member here: the file ends inside one, the member is malformed, or these bytes are no BGZF member
      give_back();
      if (kr_bgzf_member_size(comp, want) != 0)
        order.fail("damaged block-gzipped file (a member is cut short or malformed at offset " + std::to_string(off) + "): " + s.query);
      else
        foreign_at = off; // an ordinary gzip member appended, say: zlib's from here on
      break;
    }
    // The chunk ends at its last record start, as a plain file's does; none, or the file's last members: it goes out whole
    bool last = off + cb >= qsize;
    uint64_t moff = cb;
    uint32_t uoff = 0;
    uint64_t c = last ? 0 : kr_bgzf_chunk_cut(comp, cb, skip, fasta_parse ? 1u : 0u, &moff, &uoff);
    if (!c && !last) { // a chunk that begins near the end of a member may hold the head of one record only: one more member's worth
      if (kr_bgzf_walk(comp, want, s.chunk_bytes + skip + 65536, &nm, &cb, &U)) error_exit(kr_last_error());
      last = off + cb >= qsize;
      moff = cb;
      c = last ? 0 : kr_bgzf_chunk_cut(comp, cb, skip, fasta_parse ? 1u : 0u, &moff, &uoff);
    }
    const uint64_t comp_len = !c ? cb : uoff ? moff + kr_bgzf_member_size(comp + moff, cb - moff) : moff;
    const uint64_t nbytes = c ? c : U - skip;
    const uint64_t next_off = c ? off + moff : off + cb;
    const uint32_t next_skip = c ? uoff : 0;
    if (nbytes == 0) { // (empty members only: the end-of-file marker)
      give_back();
      off = next_off, skip = next_skip;
      continue;
    }
    std::unique_ptr<Job> j(new Job());
    j->raw = buf, j->raw_len = nbytes, j->raw_off = off, j->at_eof = last;
    j->fasta = fasta_parse, j->closed = last || (fasta_parse && c);
    j->comp = comp, j->comp_len = comp_len, j->skip = skip;
    for (uint64_t p = 0, u = 0; p < comp_len;) {
      const uint32_t ms = kr_bgzf_member_size(comp + p, comp_len - p);
      j->m_off.push_back(off + p), j->m_u.push_back(u);
      u += (uint32_t)comp[p + ms - 4] | (uint32_t)comp[p + ms - 3] << 8 | (uint32_t)comp[p + ms - 2] << 16 | (uint32_t)comp[p + ms - 1] << 24;
      p += ms;
      if (p >= comp_len) j->m_off.push_back(off + p), j->m_u.push_back(u);
    }
    off = next_off, skip = next_skip;
    enqueue(std::move(j));
  }
  ns_parse += since(t_parse);
  chunks_done(foreign_at);
}

// the host reader: batches of parsed records, split so that they fit the stream limits
void Run::read_host()
{
  while (!order.failed()) { // (a worker without a stream, or one whose batch failed: reported at the end)
    kr_fastx_batch b;
    auto t_parse = Clock::now();
    if (kr_fastx_next(fx, s.batch_bases, &b)) error_exit(kr_last_error());
    ns_parse += since(t_parse);
    auto t_job = Clock::now();
    uint32_t r0 = 0;
    while (r0 < b.nreads) {
      uint32_t r1 = r0;
      while (r1 < b.nreads && r1 - r0 < s.max_reads && b.offsets[r1 + 1] - b.offsets[r0] <= s.max_bases) ++r1;
      if (r1 == r0) error_exit("A query sequence is longer than the supported maximum per batch");
      std::unique_ptr<Job> j(new Job());
      j->n = r1 - r0;
      if (r0 == 0 && r1 == b.nreads && !s.copy_batches) {
        // the whole batch is one job: it changes hands as it is (QSeq gives IBatch its vectors by swap, src/query.cpp:32-33); the
        // reader thread copies nothing and the worker gives the buffers back when the batch is done
        if (kr_fastx_detach(fx, &j->held)) error_exit(kr_last_error());
        j->bases = b.bases, j->offsets = b.offsets, j->names = b.names;
      } else {
        j->own_bases.assign(b.bases + b.offsets[r0], b.bases + b.offsets[r1]);
        j->own_offsets.resize(r1 - r0 + 1);
        for (uint32_t i = r0; i <= r1; ++i) j->own_offsets[i - r0] = b.offsets[i] - b.offsets[r0];
        // the reader keeps a batch's names back to back in one buffer, in order (include/krepp_amd.h)
        const char* first = b.names[r0];
        const char* last = b.names[r1 - 1];
        j->own_blob.assign(first, (size_t)(last - first) + strlen(last) + 1);
        j->own_names.resize(r1 - r0);
        for (uint32_t i = r0; i < r1; ++i) j->own_names[i - r0] = j->own_blob.data() + (b.names[i] - first);
        j->bases = j->own_bases.data(), j->offsets = j->own_offsets.data(), j->names = j->own_names.data();
      }
      j->blob = j->names[0];
      j->blob_bytes = (size_t)(j->names[j->n - 1] - j->names[0]) + strlen(j->names[j->n - 1]) + 1;
      j->first_read = nreads_total;
      nreads_total += r1 - r0;
      enqueue(std::move(j));
      r0 = r1;
    }
    ns_job += since(t_job);
    if (!b.more) break;
  }
}

void Run::end_of_input()
{
  if (s.timing) fprintf(stderr, "[timing] reader: end of input at %.3f s (%llu batches)\n", at(), (unsigned long long)nbatches);
  {
    std::lock_guard<std::mutex> lk(order.mu);
    eof = true;
  }
  order.cv_work.notify_all();
  order.close(nbatches);
}

// every thread has been joined: the summary rows, the jplace frame, the closing lines; then the process ends, or tears down
int Run::finish()
{
  const bool place = s.place, seek = s.seek;
  if (order.failed()) error_exit(order.error());
  std::string rows;
  if (s.summarize && !place) // src/krepp.cpp:388-393 (ascending colour id instead of hash-map order)
    for (uint32_t se = 0; se < wcount.size(); ++se)
      if (wcount[se] != 0) {
        char row[64];
        std::string line = kr_host_index_node_name(hx, se);
        snprintf(row, sizeof(row), "\t%.5f\t%.5f\n", wcount[se], wcount[se] / twcount);
        rows += line + row;
      }
  if (s.tabular == 2) { // src/krepp.cpp:493-497
    char* t = nullptr;
    uint64_t l = 0;
    if (kr_place_summary_add(ptree, carry.data(), carry.size(), pwcount.data(), &ptwcount) ||
        kr_place_summary_text(ptree, pwcount.data(), ptwcount, &t, &l))
      error_exit(kr_last_error());
    rows.append(t, l);
    kr_free(t);
  }
  if (place) {
    char* t = nullptr;
    uint64_t l = 0;
    if (kr_place_frame(ptree, 1, s.tabular, s.invocation.c_str(), nreads_total, &t, &l)) error_exit(kr_last_error());
    rows.append(t, l);
    kr_free(t);
    kr_place_tree_free(ptree);
  }
  if (!rows.empty()) put(rows.data(), rows.size()); // (only where no worker wrote side by side: the stream's position is the file's end)
  order.rewind_to_end(out);
  if (s.bgzf_out) { // the end member, once, last
    uint8_t eof_member[28];
    kr_bgzf_eof(eof_member);
    fwrite(eof_member, 1, sizeof(eof_member), out);
  }
  if (out != stdout) fclose(out);
  if (out2) {
    if (s.bgzf_out) {
      uint8_t eof_member[28];
      kr_bgzf_eof(eof_member);
      fwrite(eof_member, 1, sizeof(eof_member), out2);
    }
    if (fclose(out2) != 0) error_exit("Failed to write " + s.output2);
  }
  for (FILE* f : {ex_matched, ex_unmatched, ex_matched2, ex_unmatched2}) {
    if (!f) continue;
    if (s.extract_bgzf) { // the end member, once, last
      uint8_t eof_member[28];
      kr_bgzf_eof(eof_member);
      fwrite(eof_member, 1, sizeof(eof_member), f);
    }
    if (fclose(f) != 0) error_exit("Failed to write an --extract-* file");
  }
  const double sec = at();
  fprintf(stderr, place ? "Done placing queries, elapsed: %g sec (%.0f reads/s on %d GPU(s))\n" : seek ? "Done seeking query sequences, elapsed: %g sec (%.0f reads/s on %d GPU(s))\n" : "Done estimating distances, elapsed: %g sec (%.0f reads/s on %d GPU(s))\n", sec,
          sec > 0 ? nreads_total / sec : 0.0, s.ngpus);
  if (s.timing)
    fprintf(stderr, "[timing] parse %.3f s, job hand-over (incl. waiting for queue space) %.3f s, device %.3f s, format %.3f s, write %.3f s; of the elapsed time, until the last worker had its stream and page-locked buffers: %.3f s (the reader parses meanwhile)\n",
            ns_parse / 1e9, ns_job / 1e9, ns_dev / 1e9, ns_fmt / 1e9, ns_write / 1e9, std::chrono::duration<double>(t_loop - t_init).count());
  if (s.timing && s.gpu_seek) fprintf(stderr, "[timing] gpu-seek: %llu reads through the seek kernels\n", (unsigned long long)nreads_seek.load());
  if (s.timing && s.extract())
    fprintf(stderr, "[timing] extract: %llu matched of %llu reads, %llu + %llu bytes, %.3f ms of kernels\n", (unsigned long long)ex_nmatched.load(), (unsigned long long)ex_reads.load(),
            (unsigned long long)ex_bytes_m.load(), (unsigned long long)ex_bytes_u.load(), ex_kernel_us.load() / 1e3);
  if (s.timing && s.paired())
    fprintf(stderr, "[timing] extract pairs: %llu matched of %llu pairs (rule %s), %llu bytes, %.3f ms of kernels\n", (unsigned long long)ex_pairs_matched.load(),
            (unsigned long long)ex_pairs.load(), s.pair_rule == KR_PAIR_ANY ? "any" : "both", (unsigned long long)ex_pair_bytes.load(), ex_pair_kernel_us.load() / 1e3);
  if (s.timing && gpu_parse)
    fprintf(stderr, "[timing] gpu-parse: %llu %s records found on the device\n", (unsigned long long)nreads_dev.load(), fasta_parse ? "FASTA" : "FASTQ");
  if (s.timing && gz) {
    uint64_t c[11] = {0};
    (void)kr_gzdev_counters(gz, c);
    fprintf(stderr, "[timing] gpu-inflate: %llu super-chunks, %llu sub-chunks linked, %llu without a start, %llu dropped, host ranges %llu; kernels: search %.1f ms, decode %.1f ms, chain %.1f ms, resolve %.1f ms; copies %.1f ms; %llu compressed bytes taken in twice\n",
            (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3], (unsigned long long)c[4], c[6] / 1e3, c[7] / 1e3, c[8] / 1e3, c[9] / 1e3, c[10] / 1e3, (unsigned long long)c[5]);
  }
  if (s.timing && s.plain_dist()) // (a batch split at capacity counts once per piece)
    fprintf(stderr, "[timing] report text: %llu batches written from device text, %llu through the host formatter\n", (unsigned long long)nb_dev_text.load(),
            (unsigned long long)nb_host_text.load());
  if (s.gpu_deflate) { // place pieces: the ranges the library deflated on the device / by its host encoder
    uint64_t dev_ranges = 0, host_ranges = 0;
    kr_place_bgzf_counters(&dev_ranges, &host_ranges);
    n_dev_deflate += dev_ranges, n_host_deflate += host_ranges;
  }
  if (s.timing && s.bgzf_out)
    fprintf(stderr, "[timing] bgzf-out: %llu text bytes, %llu compressed bytes (without the end member); %llu pieces deflated on the device, %llu by the host encoder; level %u\n",
            (unsigned long long)nb_plain.load(), (unsigned long long)nb_comp.load(), (unsigned long long)n_dev_deflate.load(), (unsigned long long)n_host_deflate.load(), s.bgzf_level);
  fprintf(stderr, "Total number of sequences queried: %llu\n", (unsigned long long)nreads_total);
  // Everything is written.  Unmapping 19 GB of index, 10 GB of host tables and the page-locked buffers one by one takes 0.8-1.2 s
  // that nobody is waiting for: the process ends here and the kernel reclaims the lot (KR_CLI_CLEAN_EXIT=1: free everything in
  // order -- leak checkers, tests of the tear-down path).
  if (!s.clean_exit) {
    fflush(stdout);
    fflush(stderr);
    _exit(0);
  }
  auto t_down = Clock::now();
  kr_fastx_close(fx); // (the reader's thread pool and chunk buffers)
  kr_gzdev_close(gz);
  for (kr_stream* st : streams_to_free) kr_stream_destroy(st);
  for (auto* d : dix) kr_index_free(d);
  kr_host_index_free(hx);
  if (s.timing) fprintf(stderr, "[timing] tear-down %.3f s\n", since(t_down) / 1e9);
  return 0;
}

// reader (this thread) -> one worker per stream, each GPU with its own replica of the index -> writer, in input order
static int run_query(const Args& a, const std::string& invocation, int mode)
{
  const Settings s = resolve_settings(a, invocation, mode);
  Run r(s);
  r.start_up(a);
  r.open_input();
  std::vector<std::thread> workers;
  for (int w = 0; w < s.nworkers; ++w) workers.emplace_back([&r, w] { Worker(r, w % r.s.ngpus).loop(); });
  std::thread writer([&r] { r.write_loop(); });
  if (s.seek) fprintf(stderr, "Seeking query sequences in the sketch...\n");
  if (!s.place && !s.seek) fprintf(stderr, "Estimating distances between given sequences and references...\n");
  if (s.paired())
    r.read_pairs();
  else if (r.gpu_parse)
    r.gz ? r.read_chunks_gzip() : r.bgzf ? r.read_chunks_bgzf() : r.read_chunks();
  if (r.fx) r.read_host();
  r.end_of_input();
  for (auto& w : workers) w.join();
  writer.join();
  return r.finish();
}

// --gpu-minimizers / --gpu-keys / --device of `index` and `sketch`: kr_build_params::gpu_minimizers is a bit set, the key stage implies the leaf stage
// (--gpu-colours, which implies both, is `index`'s alone: run_index)
static void gpu_build_options(const Args& a, kr_build_params& bp)
{
  auto on = [&](const char* f) { return a.flag.count(f) && a.flag.at(f); };
  bp.gpu_minimizers = on("--gpu-minimizers") ? KR_BUILD_GPU_MINIMIZERS : 0u;
  if (on("--gpu-keys")) bp.gpu_minimizers |= KR_BUILD_GPU_MINIMIZERS | KR_BUILD_GPU_KEYS;
  bp.device = a.has("--device") ? atoi(a.get("--device").c_str()) : 0;
}

// --sdust-t / --sdust-w (src/krepp.cpp:530-531,576-577): non-negative integers, masking on when both are positive, and then the
// two lines of validate_configuration (src/krepp.hpp:80-83)
static void sdust_options(const Args& a, kr_build_params& bp)
{
  auto value = [&](const char* name) -> uint32_t {
    if (!a.has(name)) return 0;
    const std::string v = a.get(name);
    char* end = nullptr;
    const long long n = strtoll(v.c_str(), &end, 10);
    if (v.empty() || *end || n < 0 || n > 0x7FFFFFFFll) error_exit(std::string(name) + ": a non-negative integer is required");
    return (uint32_t)n;
  };
  bp.sdust_t = value("--sdust-t");
  bp.sdust_w = value("--sdust-w");
  if (bp.sdust_t != 0 && bp.sdust_w != 0) {
    fprintf(stderr, "Setting --sdust-w and --sdust-t to >0 will enable dustmasker.\n");
    fprintf(stderr, "With dustmasker, krepp might fail to model subsampling and be slightly inaccurate.\n");
  }
}

static int run_index(const Args& a)
{
  // the reference's `index` takes -i,--input-file (name<TAB>path map) and -o,--index-dir
  // (src/krepp.cpp:563-566); the shared short-option table maps -i/-o to the dist names.
  std::string input, outdir;
  if (a.has("--input-file")) {
    input = a.get("--input-file");
    outdir = a.has("--index-dir") ? a.get("--index-dir") : a.get("--output-path");
  } else {
    input = a.get("--index-dir");
    outdir = a.get("--output-path");
  }
  if (input.empty() || outdir.empty()) error_exit("index requires -i/--input-file and -o/--index-dir");
  kr_build_params bp;
  memset(&bp, 0, sizeof(bp));
  bp.k = 29, bp.w = 35, bp.h = 13, bp.m = 4, bp.r = 1, bp.frac = 1; // src/krepp.hpp:47-58
  if (a.has("--kmer-len")) bp.k = (uint32_t)atoi(a.get("--kmer-len").c_str());
  bool w_given = a.has("--win-len");
  if (w_given) bp.w = (uint32_t)atoi(a.get("--win-len").c_str());
  if (a.has("--num-positions")) bp.h = (uint32_t)atoi(a.get("--num-positions").c_str());
  if (!w_given) { // src/krepp.cpp:579-582
    bp.w = bp.k + 6;
    if (!a.has("--num-positions")) bp.h = bp.k - 16;
  }
  if (a.has("--modulo-lsh")) bp.m = (uint32_t)atoi(a.get("--modulo-lsh").c_str());
  if (a.has("--residue-lsh")) bp.r = (uint32_t)atoi(a.get("--residue-lsh").c_str());
  if (a.flag.count("--frac")) bp.frac = a.flag.at("--frac");
  bp.num_threads = a.has("--num-threads") ? (uint32_t)atoi(a.get("--num-threads").c_str()) : 1;
  bp.seed = a.has("--seed") ? (uint32_t)atoi(a.get("--seed").c_str()) : 0;
  gpu_build_options(a, bp);
  if (a.flag.count("--gpu-colours") && a.flag.at("--gpu-colours")) // (`index` only: a sketch has one leaf and no colours to fold)
    bp.gpu_minimizers |= KR_BUILD_GPU_MINIMIZERS | KR_BUILD_GPU_KEYS | KR_BUILD_GPU_COLOURS;
  sdust_options(a, bp);
  fprintf(stderr, "Building the index...\n");
  std::string nwk = a.get("--nwk-file");
  if (kr_build_index(input.c_str(), nwk.empty() ? nullptr : nwk.c_str(), outdir.c_str(), &bp)) error_exit(kr_last_error());
  fprintf(stderr, "Done converting & saving\n");
  return 0;
}

static int run_sketch(const Args& a)
{ // SketchSingle (src/krepp.cpp:516-541): -i,--input-file  -o,--output-path; defaults k 26, w k+6, h k-16, m 4, r 1, frac
  const std::string input = a.has("--input-file") ? a.get("--input-file") : a.get("--index-dir");
  const std::string outp = a.get("--output-path");
  if (input.empty() || outp.empty()) error_exit("sketch requires -i/--input-file and -o/--output-path");
  kr_build_params bp;
  memset(&bp, 0, sizeof(bp));
  bp.k = 26, bp.m = 4, bp.r = 1, bp.frac = 1;
  if (a.has("--kmer-len")) bp.k = (uint32_t)atoi(a.get("--kmer-len").c_str());
  bp.w = bp.k + 6, bp.h = bp.k - 16; // src/krepp.cpp:533-536 (and the defaults [k+6], [k-16])
  if (a.has("--win-len")) {
    bp.w = (uint32_t)atoi(a.get("--win-len").c_str());
    bp.h = a.has("--num-positions") ? (uint32_t)atoi(a.get("--num-positions").c_str()) : 10; // h keeps its default
  }
  if (a.has("--modulo-lsh")) bp.m = (uint32_t)atoi(a.get("--modulo-lsh").c_str());
  if (a.has("--residue-lsh")) bp.r = (uint32_t)atoi(a.get("--residue-lsh").c_str());
  if (a.flag.count("--frac")) bp.frac = a.flag.at("--frac");
  bp.seed = a.has("--seed") ? (uint32_t)atoi(a.get("--seed").c_str()) : 0;
  gpu_build_options(a, bp);
  sdust_options(a, bp);
  fprintf(stderr, "Initializing the sketch...\n");
  if (kr_build_sketch(input.c_str(), outp.c_str(), &bp)) error_exit(kr_last_error());
  fprintf(stderr, "Done sketching & saving\n");
  return 0;
}

// `inspect` (src/krepp.cpp:696-701, Index::display_info): the host index, its statistics -- on the host, or with --gpu-stats on the
// device -- and the text, to stdout.  Without the flag no HIP call is made.
static int run_inspect(const Args& a)
{
  const std::string dir = a.get("--index-dir");
  if (dir.empty()) error_exit("inspect requires -i/--index-dir");
  const bool gpu = a.flag.count("--gpu-stats") && a.flag.at("--gpu-stats");
  const bool timing = getenv("KR_CLI_TIMING") != nullptr;
  auto t0 = Clock::now();
  kr_host_index* hx = nullptr;
  if (kr_host_index_load(dir.c_str(), &hx)) error_exit(kr_last_error());
  kr_index_view view;
  kr_host_index_view(hx, &view);
  const uint64_t t_load = since(t0);
  t0 = Clock::now();
  kr_index_stats st;
  const int rc = gpu ? kr_index_stats_device(&view, a.has("--device") ? atoi(a.get("--device").c_str()) : 0, KR_VIEW_HOST, &st)
                     : kr_index_stats_cpu(&view, KR_VIEW_HOST, &st);
  if (rc) error_exit(kr_last_error());
  const uint64_t t_stats = since(t0);
  t0 = Clock::now();
  char* text = nullptr;
  uint64_t len = 0;
  if (kr_format_inspect(hx, &st, &text, &len)) error_exit(kr_last_error());
  if (fwrite(text, 1, len, stdout) != len || fflush(stdout) != 0) error_exit("Failed to write the report");
  const uint64_t t_text = since(t0);
  if (timing) {
    uint64_t dbg[8] = {0};
    if (gpu) kr_debug_index_stats(dbg);
    fprintf(stderr, "[timing] inspect: load %.3f s, statistics %.3f s (%s), text %.3f s\n", t_load * 1e-9, t_stats * 1e-9,
            !gpu ? "host" : dbg[0] == 1 ? "device" : "device asked, host for memory", t_text * 1e-9);
  }
  kr_free(text);
  kr_index_stats_free(&st);
  kr_host_index_free(hx);
  return 0;
}

int main(int argc, char** argv)
{
  // more hardware queues than the runtime's default of 4: with two workers per GPU (each a kr_stream with its own HIP
  // streams) every stream after the third would share the last queue, and copies queued there turn into blit kernels
  // behind the other worker's kernels instead of SDMA transfers beside them.  Before the first HIP call.
  setenv("GPU_MAX_HW_QUEUES", "8", 0);
  // batches allocate and free tens of MB of rows and text over and over: keep that memory in the heap instead of
  // mapping and unmapping it each time (page faults and mmap locking showed up as 50 ms stalls per batch)
  if (!getenv("KR_CLI_DEFAULT_MALLOC")) {
    mallopt(M_MMAP_THRESHOLD, 1 << 30);
    mallopt(M_TRIM_THRESHOLD, -1);
  }
  fprintf(stderr, "krepp version: " KREPP_VERSION " (krepp-amd, MI355X)\n"); // PRINT_VERSION, src/common.hpp:51
  Args a = parse(argc, argv);
  std::string invocation;
  for (int i = 0; i < argc; ++i) invocation += std::string(argv[i]) + (i + 1 < argc ? " " : "");
  std::time_t now = std::time(nullptr);
  fprintf(stderr, "Invocation: %s\n%s", invocation.c_str(), std::ctime(&now));
  int rc;
  if (a.sub == "dist")
    rc = run_query(a, invocation, 0);
  else if (a.sub == "place")
    rc = run_query(a, invocation, 1);
  else if (a.sub == "seek")
    rc = run_query(a, invocation, 2);
  else if (a.sub == "index")
    rc = run_index(a);
  else if (a.sub == "sketch")
    rc = run_sketch(a);
  else if (a.sub == "inspect")
    rc = run_inspect(a);
  else
    error_exit("A subcommand is required (dist | place | seek | index | sketch | inspect)");
  now = std::time(nullptr);
  fprintf(stderr, "%s", std::ctime(&now));
  return rc;
}
