// pagerank -- process-level drop-in for the Sparky.java Spark job (C++ host).
//
//   pagerank <input-path> [iterations=10] [--format=edges|ccjson] [--out DIR]
//            [--save-every-iter] [--dangling=local|none|seeds] [--device N] [--quiet] [--stats]
//            [--resume DIR/PageRank<i>] [--devices D0,D1,...] [--top K] [--seeds FILE]
//            [--seed-set FILE]... [--exclude-seeds] [--tol X] [--seed-queue LISTFILE [--slots W]]
//            [--dangling-to-seeds] [--mix W0,W1,...]...
//
// Input (libpagerank_host): "src dst" edge list ("src" alone = record without links), or
// --format=ccjson "url<TAB>json" Common Crawl metadata records (Sparky.java:61-123).  URLs are
// interned to dense int32 IDs in first-appearance order, then libpagerank_hip builds the graph
// (Sparky.java:124-184) and runs the iteration (Sparky.java:164-238) on the GPU.
// Output: "Starting iter<i>" before each iteration (Sparky.java:188), then one
// "<url> has rank: <r>." line per URL (north_star); --out DIR writes DIR/PageRank<i>/part-00000
// "(url,rank)" + _SUCCESS (Sparky.java:237) for the last (or every) iteration.
// --resume DIR/PageRank<i>: start from the ranks a previous run (or Sparky.java:237) saved there
// instead of 1.0 (Sparky.java:165-170) and continue the same loop: iterations i+1 .. N-1, with
// the same "Starting iter" lines and PageRank<iter> numbering.  A directory not named
// PageRank<i> starts the loop at 0.
// --devices D0,D1,...: one row part per listed GPU (a device may repeat), driven from this one
// process by the pr_group_* API; the parts exchange contributions by device copies (xGMI peer
// copies between GPUs).  Same outputs as one GPU.
// --top K: the final listing is only the K highest-ranked URLs, rank descending, ties by first
// appearance in the input (= ID ascending), selected on the GPU (pr_get_topk / pr_group_topk).
// Without --out the rank vector never crosses to the host; --out still writes complete part files.
// --seeds FILE: personalised PageRank.  FILE lists the seed URLs, one "url" or "url weight" per line
// (weight > 0, default 1; blank lines and '#' lines skipped): the teleport mass 0.15 N goes to the
// seeds in proportion to their weights and every other URL's teleport term is 0
// (prh_seed_teleport, pr_set_teleport_sparse); the dangling term stays uniform unless --dangling=seeds
// is given.  The file is read and checked before the graph is created: a bad one exits with status 2
// without touching a GPU.  Combines with every other option; outputs have the same form as without it.
//   pagerank edges.txt 20 --seeds seeds.txt --top 100
// --dangling=seeds (needs --seeds, else a usage error before any GPU work): the run's dangling mass
// returns to the --seeds set in proportion to the weights, instead of being spread over all URLs
// (pr_set_teleport_dangling, PR_TELEPORT_DANGLING_TELEPORT): textbook personalised PageRank, in which
// a URL the seeds cannot reach drains to 0.  The graph counts its dangling mass as with
// --dangling=local.  Works with --devices, --top, --out and --resume; output format unchanged.  For
// --seed-set and --seed-queue the same choice is --dangling-to-seeds.
//   pagerank edges.txt 20 --seeds seeds.txt --dangling=seeds --top 100
// --seed-set FILE (1 to 16 times): batched personalised PageRank.  Every FILE is a seed file as for
// --seeds and gives one personalised ranking; all of them run as one batch (pr_batch_*), one pass
// over the graph per iteration for all sets.  Per set, in command-line order, the listing is a line
// "# seed set <j>: <FILE>" followed by that set's "<url> has rank: <r>." lines (with --top K its K
// best; the listings of all sets come from one select, pr_batch_get_topk_all); --out DIR writes
// DIR/seedset<j>/PageRank<last>/part-00000 + _SUCCESS.
// Not with --seeds, --devices, --resume or --save-every-iter (usage errors, before any GPU work).
//   pagerank edges.txt 20 --seed-set alice.txt --seed-set bob.txt --top 100
// --exclude-seeds (needs --seed-set and --top, else a usage error before any GPU work): every set's
// own seed URLs are left out of that set's --top listing (pr_batch_set_exclude); part files from
// --out stay complete.
//   pagerank edges.txt 20 --seed-set alice.txt --seed-set bob.txt --top 100 --exclude-seeds
// --tol X (needs --seed-set, else a usage error before any GPU work; X a finite number >= 0): every
// set stops at its own convergence, decided on the GPU (pr_batch_step_until): a set is done after the
// first iteration whose L1 delta, on the unnormalised ranks, is at most X, and the iterations argument
// becomes the cap.  "Starting iter<i>" is printed for every i below the largest count; after each
// "# seed set <j>: <FILE>" line comes "# iterations: <n_j> (converged)" or "(not converged)"; --out
// writes set j to DIR/seedset<j>/PageRank<n_j - 1>.  Each listing is that of the same command without
// --tol run for exactly n_j iterations.
//   pagerank edges.txt 500 --seed-set alice.txt --seed-set bob.txt --top 100 --tol 1e-6
// --seed-queue LISTFILE (needs --tol and --top; not with --seeds, --seed-set, --devices, --resume or
// --save-every-iter; usage errors before any GPU work): LISTFILE names one seed file per line (blank
// lines and '#' comments skipped), any number of them.  The sets are served by --slots W (1..16,
// default min(16, sets)) batch columns through pr_batch_run_queue: a column whose set has converged
// (or has had `iterations` iterations of its own) takes the next set at once.  No "Starting iter"
// lines; per set, in queue order: "# seed set <q>: <FILE>", "# iterations: <n> (converged)" or
// "(not converged)", then its --top listing (with --exclude-seeds without its own seeds) -- the lines
// --seed-set FILE --tol X --top K prints for that file alone.  --out DIR writes set q to
// DIR/seedset<q>/PageRank<n - 1>.
//   pagerank edges.txt 500 --seed-queue sets.txt --tol 1e-6 --top 100 --slots 16
// --dangling-to-seeds (needs --seed-set or --seed-queue, else a usage error before any GPU work): every
// set's dangling mass returns to that set's own seeds, in proportion to their weights
// (pr_batch_set_dangling, PR_BATCH_DANGLING_TELEPORT), instead of being spread over all URLs: a URL the
// seeds cannot reach keeps rank 0.  A set whose teleport terms sum to 0 or overflow keeps the uniform term; with
// --dangling=none there is no dangling mass and the option changes nothing.  The mode is the whole
// run's, not a set's; for --seeds (the engine's own iteration) the same choice is --dangling=seeds.
// Output format unchanged.
//   pagerank edges.txt 20 --seed-set alice.txt --seed-set bob.txt --top 100 --dangling-to-seeds
// --mix W0,W1,... (1 to 16 times; needs --seed-set and --top, not with --seed-queue; exactly one finite
// number per --seed-set file; anything else is a usage error before any GPU work): after the per-set
// listings, mix i prints "# mix <i>: <the weights as given>" and the --top listing of the blend
// sum_j W_j * ranks_j of the sets' rankings, all mixes from one pr_batch_mix_topk call and no further
// iteration.  Negative weights are allowed (1,-0.25: what set 0 ranks highly and set 1 does not).  With
// --exclude-seeds a mix leaves out the seeds of every set it gives a non-zero weight.  The per-set
// output is that of the run without --mix.
//   pagerank edges.txt 20 --seed-set alice.txt --seed-set bob.txt --top 100 --mix 0.5,0.5 --mix 1,-0.25
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "pagerank_hip.h"
#include "pagerank_host.h"

namespace {

struct Options {
  std::string path, out, resume, seeds;
  int iterations = 10;  // Sparky.java:187
  int format = PRH_FORMAT_EDGES;
  bool save_every = false, quiet = false, stats = false;
  bool exclude_seeds = false;  // --exclude-seeds
  bool dangling_to_seeds = false;  // --dangling-to-seeds
  bool dangling_seeds = false;     // --dangling=seeds (flags stay PR_DANGLING_LOCAL)
  bool has_tol = false;        // --tol X: `iterations` is the cap
  double tol = 0.0;
  uint32_t flags = PR_DANGLING_LOCAL;
  int device = 0;
  int top = 0;  // --top K (0: list every URL)
  std::vector<int> devices;  // --devices: one part per entry (empty: one part on `device`)
  std::vector<std::string> seed_sets;  // --seed-set, in command-line order (empty: no batch)
  std::string seed_queue;              // --seed-queue LISTFILE (empty: no queue)
  int slots = 0;                       // --slots W (0: min(16, queries))
  std::vector<std::string> mixes;      // --mix, as given, in command-line order
  std::vector<double> mix_weights;     // mixes.size() x seed_sets.size(), row-major
};

std::vector<int> parse_devices(const std::string &s) {
  std::vector<int> d;
  size_t i = 0;
  while (i <= s.size()) {
    const size_t j = s.find(',', i);
    const std::string t = s.substr(i, j == std::string::npos ? std::string::npos : j - i);
    if (t.empty() || t.find_first_not_of("0123456789") != std::string::npos) return {};
    d.push_back(std::atoi(t.c_str()));
    if (j == std::string::npos) break;
    i = j + 1;
  }
  return d;
}

[[noreturn]] void usage(const char *msg) {
  if (msg) std::fprintf(stderr, "pagerank: %s\n", msg);
  std::fprintf(stderr,
               "usage: pagerank <input-path> [iterations=10] [--format=edges|ccjson] [--out DIR]\n"
               "                [--save-every-iter] [--dangling=local|none|seeds] [--device N] [--quiet] [--stats]\n"
               "                [--resume DIR/PageRank<i>] [--devices D0,D1,...] [--top K] [--seeds FILE]\n"
               "                (--dangling=seeds, with --seeds: the dangling mass returns to the seeds instead of all\n"
               "                URLs)\n"
               "                [--seed-set FILE]...  (1 to 16 seed files, run as one batch; not with --seeds,\n"
               "                --devices, --resume or --save-every-iter)\n"
               "                [--exclude-seeds]  (with --seed-set and --top: a set's own seeds are left out of\n"
               "                its listing)\n"
               "                [--tol X]  (with --seed-set: every set stops once its L1 delta is <= X; iterations\n"
               "                is the cap)\n"
               "                [--seed-queue LISTFILE --tol X --top K [--slots W]]  (one seed-file path per line, any\n"
               "                number of them, served by W = 1..16 batch columns that are refilled as sets converge;\n"
               "                not with --seeds, --seed-set, --devices, --resume or --save-every-iter)\n"
               "                [--dangling-to-seeds]  (with --seed-set or --seed-queue: a set's dangling mass returns to\n"
               "                its own seeds instead of all URLs; a set whose teleport terms sum to 0 or overflow keeps the\n"
               "                uniform term; the whole run's mode, not a set's; for --seeds: --dangling=seeds)\n"
               "                [--mix W0,W1,...]...  (with --seed-set and --top, 1 to 16 times: also list the K best\n"
               "                URLs of the weighted blend of the sets' rankings, one finite weight per --seed-set;\n"
               "                not with --seed-queue)\n");
  std::exit(2);
}

// --mix: n comma-separated finite numbers in plain decimal or exponent form, appended to *out.
bool parse_mix(const std::string &text, size_t n, std::vector<double> *out) {
  size_t i = 0, count = 0;
  while (i <= text.size()) {
    const size_t j = text.find(',', i);
    const std::string t = text.substr(i, j == std::string::npos ? std::string::npos : j - i);
    if (t.empty() || t.find_first_not_of("0123456789+-.eE") != std::string::npos) return false;
    char *end = nullptr;
    const double w = std::strtod(t.c_str(), &end);
    if (*end != '\0' || !std::isfinite(w)) return false;
    out->push_back(w);
    ++count;
    if (j == std::string::npos) break;
    i = j + 1;
  }
  return count == n;
}

Options parse(int argc, char **argv) {
  Options o;
  int pos = 0;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a == "--out" && i + 1 < argc) o.out = argv[++i];
    else if (a.rfind("--out=", 0) == 0) o.out = a.substr(6);
    else if (a == "--format=edges") o.format = PRH_FORMAT_EDGES;
    else if (a == "--format=ccjson") o.format = PRH_FORMAT_CCJSON;
    else if (a == "--save-every-iter") o.save_every = true;
    else if (a == "--quiet") o.quiet = true;
    else if (a == "--stats") o.stats = true;
    else if (a == "--exclude-seeds") o.exclude_seeds = true;
    else if (a == "--dangling-to-seeds") o.dangling_to_seeds = true;
    else if (a == "--dangling=local") o.flags = PR_DANGLING_LOCAL, o.dangling_seeds = false;
    else if (a == "--dangling=none") o.flags = PR_DANGLING_NONE, o.dangling_seeds = false;
    else if (a == "--dangling=seeds") o.flags = PR_DANGLING_LOCAL, o.dangling_seeds = true;
    else if (a == "--device" && i + 1 < argc) o.device = std::atoi(argv[++i]);
    else if (a == "--resume" && i + 1 < argc) o.resume = argv[++i];
    else if (a.rfind("--resume=", 0) == 0) o.resume = a.substr(9);
    else if (a == "--seeds" && i + 1 < argc) o.seeds = argv[++i];
    else if (a.rfind("--seeds=", 0) == 0) o.seeds = a.substr(8);
    else if (a == "--seed-set" && i + 1 < argc) o.seed_sets.push_back(argv[++i]);
    else if (a.rfind("--seed-set=", 0) == 0) o.seed_sets.push_back(a.substr(11));
    else if (a == "--mix" && i + 1 < argc) o.mixes.push_back(argv[++i]);
    else if (a.rfind("--mix=", 0) == 0) o.mixes.push_back(a.substr(6));
    else if (a == "--mix") usage("--mix takes one finite weight per --seed-set, separated by commas");
    else if (a == "--seed-queue" && i + 1 < argc) o.seed_queue = argv[++i];
    else if (a.rfind("--seed-queue=", 0) == 0) o.seed_queue = a.substr(13);
    else if ((a == "--slots" && i + 1 < argc) || a.rfind("--slots=", 0) == 0) {
      const std::string t = a == "--slots" ? std::string(argv[++i]) : a.substr(8);
      if (t.empty() || t.size() > 2 || t.find_first_not_of("0123456789") != std::string::npos || std::atoi(t.c_str()) < 1 ||
          std::atoi(t.c_str()) > 16)
        usage("--slots takes a count W in 1..16");
      o.slots = std::atoi(t.c_str());
    }
    else if ((a == "--devices" && i + 1 < argc) || a.rfind("--devices=", 0) == 0) {
      o.devices = parse_devices(a == "--devices" ? std::string(argv[++i]) : a.substr(10));
      if (o.devices.empty()) usage("--devices takes a comma-separated list of device numbers");
    }
    else if ((a == "--top" && i + 1 < argc) || a.rfind("--top=", 0) == 0) {
      const std::string t = a == "--top" ? std::string(argv[++i]) : a.substr(6);
      if (t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos || std::atoi(t.c_str()) < 1)
        usage("--top takes a count K >= 1");
      o.top = std::atoi(t.c_str());
    }
    else if ((a == "--tol" && i + 1 < argc) || a.rfind("--tol=", 0) == 0) {
      const std::string t = a == "--tol" ? std::string(argv[++i]) : a.substr(6);
      char *end = nullptr;
      o.tol = std::strtod(t.c_str(), &end);
      if (t.empty() || *end != '\0' || !std::isfinite(o.tol) || !(o.tol >= 0.0)) usage("--tol: not a finite number >= 0");
      o.has_tol = true;
    }
    else if (a == "-h" || a == "--help") usage(nullptr);
    else if (!a.empty() && a[0] == '-') usage(("unknown option " + a).c_str());
    else if (pos == 0) { o.path = a; ++pos; }
    else if (pos == 1) { o.iterations = std::atoi(a.c_str()); ++pos; }
    else usage("too many positional arguments");
  }
  if (o.path.empty()) usage("missing input path");
  if (o.iterations < 0) usage("iterations must be >= 0");
  if (o.dangling_to_seeds && o.seed_sets.empty() && o.seed_queue.empty())
    usage("--dangling-to-seeds needs --seed-set or --seed-queue");
  if (o.dangling_seeds && o.seeds.empty())
    usage(o.seed_sets.empty() && o.seed_queue.empty()
              ? "--dangling=seeds needs --seeds"
              : "--dangling=seeds needs --seeds; with --seed-set or --seed-queue use --dangling-to-seeds");
  if (!o.mixes.empty()) {
    if (!o.seed_queue.empty()) usage("--mix does not combine with --seed-queue");
    if (o.seed_sets.empty() || o.top == 0) usage("--mix needs --seed-set and --top");
    if (o.mixes.size() > 16) usage("--mix: at most 16 mixes");
    for (const std::string &m : o.mixes)
      if (!parse_mix(m, o.seed_sets.size(), &o.mix_weights))
        usage("--mix takes one finite weight per --seed-set, separated by commas");
  }
  if (!o.seed_queue.empty()) {
    if (!o.seeds.empty() || !o.seed_sets.empty() || !o.devices.empty() || !o.resume.empty() || o.save_every)
      usage("--seed-queue does not combine with --seeds, --seed-set, --devices, --resume or --save-every-iter");
    if (!o.has_tol || o.top == 0) usage("--seed-queue needs --tol and --top");
    if (o.iterations < 1) usage("--seed-queue: iterations (the cap of every set) must be >= 1");
    return o;
  }
  if (o.slots != 0) usage("--slots needs --seed-queue");
  if (o.exclude_seeds && (o.seed_sets.empty() || o.top == 0)) usage("--exclude-seeds needs --seed-set and --top");
  if (o.has_tol && o.seed_sets.empty()) usage("--tol needs --seed-set");
  if (!o.seed_sets.empty()) {
    if (!o.seeds.empty()) usage("--seeds and --seed-set are exclusive");
    if (o.seed_sets.size() > 16) usage("--seed-set: at most 16 seed sets");
    if (!o.devices.empty() || !o.resume.empty() || o.save_every)
      usage("--seed-set does not combine with --devices, --resume or --save-every-iter");
  }
  return o;
}

// --seeds: the seed IDs and their teleport terms (prh_seed_teleport); n == 0: a uniform run
struct Seeds {
  int32_t n = 0;
  int32_t *ids = nullptr;
  std::vector<double> values;
};

struct Job {
  const Options *opt;
  const prh_edges *edges;
  int start = 0;  // global index of the run's first iteration (--resume)
  int error = 0;
};

// i of a ".../PageRank<i>" directory (trailing '/' allowed), or -1
int saved_iteration(std::string d) {
  while (d.size() > 1 && d.back() == '/') d.pop_back();
  const size_t slash = d.rfind('/');
  const std::string base = slash == std::string::npos ? d : d.substr(slash + 1);
  if (base.rfind("PageRank", 0) != 0 || base.size() == 8) return -1;
  for (size_t k = 8; k < base.size(); ++k)
    if (base[k] < '0' || base[k] > '9') return -1;
  return std::atoi(base.c_str() + 8);
}

void on_iter(int32_t it_run, const double *ranks, double dc, double l1, double ms, void *user) {
  Job *job = static_cast<Job *>(user);
  const Options &o = *job->opt;
  const int32_t it = job->start + it_run;
  if (!o.out.empty() && ranks && (o.save_every || it == o.iterations - 1)) {
    if (prh_write_part(job->edges, o.out.c_str(), it, ranks) != 0) {
      std::fprintf(stderr, "pagerank: %s\n", prh_last_error());
      job->error = 1;
    }
  }
  if (o.stats)
    std::fprintf(stderr, "iter %d: dangling_sum=%.17g l1_delta=%.17g ms=%.3f\n", it, dc, l1, ms);
  if (it + 1 < o.iterations) std::printf("Starting iter%d\n", it + 1);
}

// --devices: build one part per device, then run the iterations as a single-process group with
// the same callback protocol as pr_run (ranks merged from every part, dc / L1 from part 0's
// stats, which sum every part's slots).
int run_group(const Options &o, const prh_edges *edges, const Seeds &seeds, const double *init, int n_run, Job *job,
              std::vector<double> *ranks, std::vector<int32_t> *top_ids, std::vector<double> *top_ranks) {
  const int P = (int)o.devices.size();
  const int32_t V = prh_n_vertices(edges);
  std::vector<pr_graph *> parts(P, nullptr);
  int rc = PR_OK;
  for (int p = 0; p < P && rc == PR_OK; ++p)
    rc = pr_graph_create_part(o.devices[p], p, P, V, prh_n_edges(edges), prh_src(edges), prh_dst(edges),
                              o.flags | PR_NO_CANONICAL, &parts[p]);
  const bool want = !o.out.empty();
  for (int p = 0; p < P && rc == PR_OK && seeds.n > 0; ++p)  // every part, the same arguments
    rc = pr_set_teleport_sparse(parts[p], seeds.n, seeds.ids, seeds.values.data(), 0.0);
  for (int p = 0; p < P && rc == PR_OK && o.dangling_seeds; ++p)  // --dangling=seeds: every part alike
    rc = pr_set_teleport_dangling(parts[p], PR_TELEPORT_DANGLING_TELEPORT);
  if (rc == PR_OK) rc = pr_group_reset(parts.data(), P, 0.15, 0.85, init);
  for (int it = 0; it < n_run && rc == PR_OK; ++it) {
    const auto t0 = std::chrono::steady_clock::now();
    rc = pr_group_step(parts.data(), P, 1);
    if (rc == PR_OK) rc = pr_group_sync(parts.data(), P);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    double st[PR_STAT_COUNT] = {0};
    if (rc == PR_OK) rc = pr_get_stats(parts[0], st, PR_STAT_COUNT);
    // ranks to the host only for a part file that is written (every iteration, or the last)
    const bool fetch = want && (o.save_every || job->start + it == o.iterations - 1);
    for (int p = 0; p < P && rc == PR_OK && fetch; ++p) rc = pr_get_ranks(parts[p], ranks->data());
    if (rc == PR_OK) on_iter(it, fetch ? ranks->data() : nullptr, st[PR_STAT_LAST_DC], st[PR_STAT_LAST_L1], ms, job);
  }
  // --top: the K best pairs instead of the whole vector (which no part file needs any more here)
  for (int p = 0; p < P && rc == PR_OK && o.top == 0; ++p) rc = pr_get_ranks(parts[p], ranks->data());
  if (rc == PR_OK && o.top > 0 && !o.quiet) {
    int32_t n = 0;
    rc = pr_group_topk(parts.data(), P, (int32_t)top_ids->size(), top_ids->data(), top_ranks->data(), &n);
    top_ids->resize(rc == PR_OK ? (size_t)n : 0);
  }
  const std::string err = rc == PR_OK ? std::string() : std::string(pr_last_error());
  for (pr_graph *g : parts)
    if (g) pr_graph_destroy(g);
  if (rc != PR_OK) std::fprintf(stderr, "pagerank: multi-GPU run failed (%d): %s\n", rc, err.c_str());
  return rc;
}

// --seed-set: every set is one column of a batch over one graph (which keeps its canonical CSR: the
// batch runs over it).  Prints the iteration lines, then per set its header and listing.
int run_seed_sets(const Options &o, const prh_edges *edges, const std::vector<Seeds> &sets) {
  const int32_t V = prh_n_vertices(edges);
  pr_graph *g = nullptr;
  pr_batch *b = nullptr;
  int rc = pr_graph_create(o.device, V, prh_n_edges(edges), prh_src(edges), prh_dst(edges), o.flags, &g);
  if (rc == PR_OK) rc = pr_batch_create(g, (int32_t)sets.size(), &b);
  if (rc == PR_OK && o.dangling_to_seeds) rc = pr_batch_set_dangling(b, PR_BATCH_DANGLING_TELEPORT);
  for (size_t j = 0; j < sets.size() && rc == PR_OK; ++j)
    rc = pr_batch_set_teleport_sparse(b, (int32_t)j, sets[j].n, sets[j].ids, sets[j].values.data(), 0.0);
  if (rc == PR_OK) rc = pr_batch_reset(b, 0.15, 0.85, nullptr);
  // iterations applied to every set: the argument, or with --tol each set's own count (the cap at most)
  std::vector<int32_t> n_it(sets.size(), o.iterations);
  std::vector<char> converged(sets.size(), 0);
  if (o.has_tol) {
    if (rc == PR_OK) rc = pr_batch_step_until(b, o.iterations, o.tol, n_it.data());
    double dc[16], l1[16];
    if (rc == PR_OK) rc = pr_batch_get_norms(b, dc, l1);
    for (size_t j = 0; j < sets.size() && rc == PR_OK; ++j) converged[j] = n_it[j] > 0 && l1[j] <= o.tol;
    const int32_t most = rc == PR_OK ? *std::max_element(n_it.begin(), n_it.end()) : 0;
    for (int32_t it = 0; it < most; ++it) std::printf("Starting iter%d\n", it);
  } else {
    for (int it = 0; it < o.iterations && rc == PR_OK; ++it) {
      std::printf("Starting iter%d\n", it);
      rc = pr_batch_step(b, 1);
    }
  }
  int error = 0;
  std::vector<double> ranks((size_t)V + 1);
  const int32_t top_k = o.top < V ? o.top : V;
  // --top: the listings of all sets from one select, set j's pairs at j * top_k
  const bool listed = o.top > 0 && !o.quiet;
  std::vector<int32_t> top_ids(listed ? (size_t)top_k * sets.size() + 1 : 1), top_n(sets.size() + 1);
  std::vector<double> top_ranks(top_ids.size());
  for (size_t j = 0; j < sets.size() && rc == PR_OK && o.exclude_seeds; ++j)  // a set's own seeds never appear in its listing
    rc = pr_batch_set_exclude(b, (int32_t)j, sets[j].n, sets[j].ids);
  if (rc == PR_OK && listed) rc = pr_batch_get_topk_all(b, top_k, top_ids.data(), top_ranks.data(), top_n.data());
  for (size_t j = 0; j < sets.size() && rc == PR_OK; ++j) {
    const bool full = !o.out.empty() || (o.top == 0 && !o.quiet);
    if (full) rc = pr_batch_get_ranks(b, (int32_t)j, ranks.data());
    if (rc == PR_OK && !o.out.empty() && n_it[j] > 0 &&
        prh_write_part(edges, (o.out + "/seedset" + std::to_string(j)).c_str(), n_it[j] - 1, ranks.data()) != 0) {
      std::fprintf(stderr, "pagerank: %s\n", prh_last_error());
      error = 1;
    }
    if (rc != PR_OK || o.quiet) continue;
    std::printf("# seed set %zu: %s\n", j, o.seed_sets[j].c_str());
    if (o.has_tol) std::printf("# iterations: %d (%s)\n", n_it[j], converged[j] ? "converged" : "not converged");
    std::fflush(stdout);
    int rc_out = 0;
    if (o.top > 0) {
      rc_out = prh_write_has_rank_ids(edges, nullptr, top_ids.data() + j * (size_t)top_k, top_ranks.data() + j * (size_t)top_k,
                                      top_n[j]);
    } else {
      rc_out = prh_write_has_rank(edges, nullptr, ranks.data());
    }
    if (rc_out != 0) {
      std::fprintf(stderr, "pagerank: %s\n", prh_last_error());
      error = 1;
    }
    std::fflush(stdout);
  }
  if (rc == PR_OK && !o.mixes.empty() && !o.quiet) {  // the listings of all mixes from one call
    const size_t n_mixes = o.mixes.size(), W = sets.size();
    // --exclude-seeds: a mix leaves out the seeds of every set it gives a non-zero weight
    std::vector<std::vector<int32_t>> excl(n_mixes);
    std::vector<int32_t> n_excl(n_mixes, 0);
    std::vector<const int32_t *> excl_ptr(n_mixes, nullptr);
    for (size_t i = 0; i < n_mixes && o.exclude_seeds; ++i) {
      for (size_t j = 0; j < W; ++j)
        if (o.mix_weights[i * W + j] != 0.0) excl[i].insert(excl[i].end(), sets[j].ids, sets[j].ids + sets[j].n);
      std::sort(excl[i].begin(), excl[i].end());
      excl[i].erase(std::unique(excl[i].begin(), excl[i].end()), excl[i].end());
      n_excl[i] = (int32_t)excl[i].size();
      excl_ptr[i] = excl[i].empty() ? nullptr : excl[i].data();
    }
    std::vector<int32_t> mix_ids((size_t)top_k * n_mixes + 1), mix_n(n_mixes);
    std::vector<double> mix_scores(mix_ids.size());
    rc = pr_batch_mix_topk(b, (int32_t)n_mixes, o.mix_weights.data(), o.exclude_seeds ? n_excl.data() : nullptr,
                           o.exclude_seeds ? excl_ptr.data() : nullptr, top_k, mix_ids.data(), mix_scores.data(),
                           mix_n.data());
    for (size_t i = 0; i < n_mixes && rc == PR_OK; ++i) {
      std::printf("# mix %zu: %s\n", i, o.mixes[i].c_str());
      std::fflush(stdout);
      if (prh_write_has_rank_ids(edges, nullptr, mix_ids.data() + i * (size_t)top_k, mix_scores.data() + i * (size_t)top_k,
                                 mix_n[i]) != 0) {
        std::fprintf(stderr, "pagerank: %s\n", prh_last_error());
        error = 1;
      }
      std::fflush(stdout);
    }
  }
  const std::string err = rc == PR_OK ? std::string() : std::string(pr_last_error());
  pr_batch_destroy(b);  // before the graph it borrows
  pr_graph_destroy(g);
  if (rc != PR_OK) {
    std::fprintf(stderr, "pagerank: --seed-set run failed (%d): %s\n", rc, err.c_str());
    return 1;
  }
  return error;
}

// --seed-queue: the list file's seed-file paths; blank lines and '#' comments are skipped.
bool read_seed_queue(const std::string &path, std::vector<std::string> *files) {
  std::FILE *f = std::fopen(path.c_str(), "r");
  if (!f) return false;
  std::string line;
  for (int c = 0; c != EOF;) {
    c = std::fgetc(f);
    if (c != EOF && c != '\n') {
      line.push_back((char)c);
      continue;
    }
    const size_t b = line.find_first_not_of(" \t\r"), e = line.find_last_not_of(" \t\r");
    if (b != std::string::npos && line[b] != '#') files->push_back(line.substr(b, e - b + 1));
    line.clear();
  }
  std::fclose(f);
  return true;
}

// What pr_batch_run_queue's callback keeps of every set: its record and its --top pairs.
struct QueueJob {
  const Options *opt = nullptr;
  const prh_edges *edges = nullptr;
  pr_batch *b = nullptr;
  int32_t top_k = 0;
  std::vector<int32_t> n_it, converged, top_n, top_ids;
  std::vector<double> top_ranks, ranks;
  int rc = PR_OK, error = 0;
};

void on_set_done(int32_t q, int32_t column, int32_t iterations, int32_t converged, double, void *user) {
  QueueJob *job = static_cast<QueueJob *>(user);
  const Options &o = *job->opt;
  job->n_it[(size_t)q] = iterations;
  job->converged[(size_t)q] = converged;
  if (job->rc != PR_OK) return;
  if (!o.quiet)
    job->rc = pr_batch_get_topk(job->b, column, job->top_k, job->top_ids.data() + (size_t)q * job->top_k,
                                job->top_ranks.data() + (size_t)q * job->top_k, &job->top_n[(size_t)q]);
  if (job->rc == PR_OK && !o.out.empty()) {
    job->rc = pr_batch_get_ranks(job->b, column, job->ranks.data());
    if (job->rc == PR_OK &&
        prh_write_part(job->edges, (o.out + "/seedset" + std::to_string(q)).c_str(), iterations - 1, job->ranks.data()) != 0) {
      std::fprintf(stderr, "pagerank: %s\n", prh_last_error());
      job->error = 1;
    }
  }
}

// --seed-queue: the sets go through the columns of one batch (pr_batch_run_queue); a column whose
// set is done is refilled at once.  Prints per set, in queue order, its header, its iteration count
// and its --top listing.
int run_seed_queue(const Options &o, const prh_edges *edges, const std::vector<std::string> &files,
                   const std::vector<Seeds> &sets) {
  const int32_t V = prh_n_vertices(edges);
  const size_t Q = sets.size();
  if (Q == 0) return 0;
  const int32_t width = o.slots > 0 ? o.slots : (int32_t)std::min<size_t>(16, Q);
  QueueJob job;
  job.opt = &o;
  job.edges = edges;
  job.top_k = o.top < V ? o.top : V;
  job.n_it.assign(Q, 0);
  job.converged.assign(Q, 0);
  job.top_n.assign(Q, 0);
  job.top_ids.assign(Q * (size_t)job.top_k + 1, 0);
  job.top_ranks.assign(Q * (size_t)job.top_k + 1, 0.0);
  job.ranks.assign((size_t)V + 1, 0.0);
  std::vector<pr_batch_query> queries(Q);
  for (size_t q = 0; q < Q; ++q)
    queries[q] = pr_batch_query{sets[q].n, sets[q].ids, sets[q].values.data(), 0.0, o.exclude_seeds ? sets[q].n : 0,
                                o.exclude_seeds ? sets[q].ids : nullptr};
  pr_graph *g = nullptr;
  int rc = pr_graph_create(o.device, V, prh_n_edges(edges), prh_src(edges), prh_dst(edges), o.flags, &g);
  if (rc == PR_OK) rc = pr_batch_create(g, width, &job.b);
  if (rc == PR_OK && o.dangling_to_seeds) rc = pr_batch_set_dangling(job.b, PR_BATCH_DANGLING_TELEPORT);
  if (rc == PR_OK) rc = pr_batch_reset(job.b, 0.15, 0.85, nullptr);
  if (rc == PR_OK) rc = pr_batch_run_queue(job.b, (int32_t)Q, queries.data(), o.iterations, o.tol, nullptr, on_set_done, &job);
  if (rc == PR_OK) rc = job.rc;
  const std::string err = rc == PR_OK ? std::string() : std::string(pr_last_error());
  pr_batch_destroy(job.b);  // before the graph it borrows
  pr_graph_destroy(g);
  if (rc != PR_OK) {
    std::fprintf(stderr, "pagerank: --seed-queue run failed (%d): %s\n", rc, err.c_str());
    return 1;
  }
  for (size_t q = 0; q < Q && !o.quiet; ++q) {
    std::printf("# seed set %zu: %s\n", q, files[q].c_str());
    std::printf("# iterations: %d (%s)\n", job.n_it[q], job.converged[q] ? "converged" : "not converged");
    std::fflush(stdout);
    if (prh_write_has_rank_ids(edges, nullptr, job.top_ids.data() + q * (size_t)job.top_k,
                               job.top_ranks.data() + q * (size_t)job.top_k, job.top_n[q]) != 0) {
      std::fprintf(stderr, "pagerank: %s\n", prh_last_error());
      job.error = 1;
    }
    std::fflush(stdout);
  }
  return job.error;
}

// The seed files `paths` read and turned into teleport terms; `what` names the option in the message.
int read_seed_files(const prh_edges *edges, const std::vector<std::string> &paths, const char *what,
                    std::vector<Seeds> *sets) {
  const int32_t V = prh_n_vertices(edges);
  sets->resize(paths.size());
  for (size_t j = 0; j < paths.size(); ++j) {
    double *weights = nullptr;
    Seeds &s = (*sets)[j];
    if (prh_read_seeds(edges, paths[j].c_str(), &s.n, &s.ids, &weights) != 0) {
      std::fprintf(stderr, "pagerank: %s %s: %s\n", what, paths[j].c_str(), prh_last_error());
      return 2;
    }
    s.values.resize((size_t)s.n);
    prh_seed_teleport(s.n, weights, 0.15, V, s.values.data());
    prh_free_seeds(nullptr, weights);
  }
  return 0;
}

}  // namespace

using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

int main(int argc, char **argv) {
  const Options o = parse(argc, argv);
  const auto t_job = Clock::now();
  prh_edges *edges = nullptr;
  if (prh_read(o.path.c_str(), o.format, &edges) != 0) {
    std::fprintf(stderr, "pagerank: %s\n", prh_last_error());
    return 1;
  }
  const int32_t V = prh_n_vertices(edges);
  Seeds seeds;
  if (!o.seeds.empty()) {  // read and checked before any graph exists: a bad file costs no GPU work
    double *weights = nullptr;
    if (prh_read_seeds(edges, o.seeds.c_str(), &seeds.n, &seeds.ids, &weights) != 0) {
      std::fprintf(stderr, "pagerank: --seeds: %s\n", prh_last_error());
      prh_free(edges);
      return 2;
    }
    seeds.values.resize((size_t)seeds.n);
    prh_seed_teleport(seeds.n, weights, 0.15, V, seeds.values.data());
    prh_free_seeds(nullptr, weights);
  }
  if (!o.seed_queue.empty()) {  // the list and every file read and checked before any graph exists
    std::vector<std::string> files;
    if (!read_seed_queue(o.seed_queue, &files)) {
      std::fprintf(stderr, "pagerank: --seed-queue %s: cannot open the list file\n", o.seed_queue.c_str());
      prh_free(edges);
      return 2;
    }
    std::vector<Seeds> sets;
    int rc = read_seed_files(edges, files, "--seed-queue", &sets);
    if (rc == 0) rc = run_seed_queue(o, edges, files, sets);
    for (Seeds &s : sets) prh_free_seeds(s.ids, nullptr);
    prh_free(edges);
    return rc;
  }
  if (!o.seed_sets.empty()) {  // every file read and checked before any graph exists
    std::vector<Seeds> sets(o.seed_sets.size());
    int rc = 0;
    for (size_t j = 0; j < sets.size() && rc == 0; ++j) {
      double *weights = nullptr;
      if (prh_read_seeds(edges, o.seed_sets[j].c_str(), &sets[j].n, &sets[j].ids, &weights) != 0) {
        std::fprintf(stderr, "pagerank: --seed-set %s: %s\n", o.seed_sets[j].c_str(), prh_last_error());
        rc = 2;
        break;
      }
      sets[j].values.resize((size_t)sets[j].n);
      prh_seed_teleport(sets[j].n, weights, 0.15, V, sets[j].values.data());
      prh_free_seeds(nullptr, weights);
    }
    if (rc == 0) rc = run_seed_sets(o, edges, sets);
    for (Seeds &s : sets) prh_free_seeds(s.ids, nullptr);
    prh_free(edges);
    return rc;
  }
  const double ms_read = ms_since(t_job);  // parse + first-appearance interning (host)
  double ms_build = 0.0, ms_run = 0.0;
  Job job{&o, edges};
  std::vector<double> ranks((size_t)V + 1), init;
  const int32_t top_k = o.top < V ? o.top : V;  // --top: K pairs at most, never more than the URLs
  std::vector<int32_t> top_ids((size_t)top_k);
  std::vector<double> top_ranks((size_t)top_k);
  if (!o.resume.empty()) {
    init.assign((size_t)V + 1, 0.0);
    if (prh_read_ranks(edges, o.resume.c_str(), init.data()) != 0) {
      std::fprintf(stderr, "pagerank: --resume: %s\n", prh_last_error());
      prh_free(edges);
      return 1;
    }
    job.start = saved_iteration(o.resume) + 1;  // 0 when the directory is not PageRank<i>
  }
  const int n_run = o.iterations > job.start ? o.iterations - job.start : 0;
  const double *init_p = init.empty() ? nullptr : init.data();
  if (o.devices.size() > 1) {
    if (n_run > 0) std::printf("Starting iter%d\n", job.start);
    const auto t0 = Clock::now();
    if (run_group(o, edges, seeds, init_p, n_run, &job, &ranks, &top_ids, &top_ranks) != PR_OK) {
      prh_free(edges);
      return 1;
    }
    ms_run = ms_since(t0);  // group: build + iterations
  } else {
    const int dev = o.devices.empty() ? o.device : o.devices[0];
    pr_graph *g = nullptr;
    auto t0 = Clock::now();
    int rc = pr_graph_create(dev, V, prh_n_edges(edges), prh_src(edges), prh_dst(edges), o.flags | PR_NO_CANONICAL, &g);
    ms_build = ms_since(t0);
    if (rc != PR_OK) {
      std::fprintf(stderr, "pagerank: graph build failed (%d): %s\n", rc, pr_last_error());
      prh_free(edges);
      return 1;
    }
    if (seeds.n > 0) rc = pr_set_teleport_sparse(g, seeds.n, seeds.ids, seeds.values.data(), 0.0);
    if (rc == PR_OK && o.dangling_seeds) rc = pr_set_teleport_dangling(g, PR_TELEPORT_DANGLING_TELEPORT);
    if (rc != PR_OK) {
      std::fprintf(stderr, "pagerank: --seeds: (%d) %s\n", rc, pr_last_error());
      pr_graph_destroy(g);
      prh_free_seeds(seeds.ids, nullptr);
      prh_free(edges);
      return 1;
    }
    if (n_run > 0) std::printf("Starting iter%d\n", job.start);
    t0 = Clock::now();
    // ranks cross PCIe only for the part files that are written: every iteration's with
    // --save-every-iter, else only the last one's, which pr_run returns in `ranks` anyway
    // (with --top and no --out not at all: the listing's K pairs come from pr_get_topk)
    const bool every = !o.out.empty() && o.save_every;
    double *final_ranks = o.top > 0 && o.out.empty() ? nullptr : ranks.data();
    rc = pr_run(g, n_run, 0.15, 0.85, init_p, final_ranks, on_iter, every ? PR_CB_RANKS : 0u, &job);
    if (rc == PR_OK && o.top > 0 && !o.quiet) {
      int32_t n = 0;
      rc = pr_get_topk(g, top_k, top_ids.data(), top_ranks.data(), &n);
      top_ids.resize(rc == PR_OK ? (size_t)n : 0);
    }
    if (rc == PR_OK && !o.out.empty() && !every && n_run > 0 &&
        prh_write_part(edges, o.out.c_str(), o.iterations - 1, ranks.data()) != 0) {
      std::fprintf(stderr, "pagerank: %s\n", prh_last_error());
      job.error = 1;
    }
    ms_run = ms_since(t0);  // iterations, with the per-iteration callback and the part-file writes
    pr_graph_destroy(g);
    if (rc != PR_OK) {
      std::fprintf(stderr, "pagerank: run failed (%d): %s\n", rc, pr_last_error());
      prh_free(edges);
      return 1;
    }
  }
  std::fflush(stdout);
  const auto t_out = Clock::now();
  const int rc_out = o.quiet   ? 0
                     : o.top > 0 ? prh_write_has_rank_ids(edges, nullptr, top_ids.data(), top_ranks.data(), (int32_t)top_ids.size())
                                 : prh_write_has_rank(edges, nullptr, ranks.data());
  if (rc_out != 0) {
    std::fprintf(stderr, "pagerank: %s\n", prh_last_error());
    job.error = 1;
  }
  std::fflush(stdout);
  const double ms_out = ms_since(t_out);
  if (o.stats)  // the job's phases (wall clock); one JSON object on stderr
    std::fprintf(stderr,
                 "{\"job\": {\"urls\": %d, \"edge_records\": %lld, \"read_intern_ms\": %.1f, \"build_ms\": %.1f, "
                 "\"iterations\": %d, \"run_ms\": %.1f, \"has_rank_out_ms\": %.1f, \"total_ms\": %.1f}}\n",
                 V, (long long)prh_n_edges(edges), ms_read, ms_build, n_run, ms_run, ms_out, ms_since(t_job));
  prh_free_seeds(seeds.ids, nullptr);
  prh_free(edges);
  return job.error;
}
