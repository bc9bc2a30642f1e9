// Test helper (stand-alone, for a -fsanitize=address,undefined build together with pr_host.cpp):
// feeds prh_parse_seeds well-formed and malformed seed files, each from a heap buffer of exactly
// len bytes -- no terminator, so a read past the end is a sanitizer report -- and every prefix of
// them (no final newline, len cut mid-token).  Checks the outcome of every case and that the
// message of a failure names the line; prints "seeds_check: done, 0 failures" and exits 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "pagerank_host.h"

namespace {

int g_failures = 0;

void expect(bool ok, const char *what, const std::string &input) {
  if (ok) return;
  ++g_failures;
  std::fprintf(stderr, "seeds_check: FAILED %s on input \"%s\" (last error: %s)\n", what, input.c_str(), prh_last_error());
}

// prh_parse_seeds over a copy of s that ends exactly at its last byte
int parse_exact(const prh_edges *e, const std::string &s, int32_t *n, int32_t **ids, double **weights) {
  char *buf = static_cast<char *>(std::malloc(s.size() ? s.size() : 1));
  if (!buf) std::abort();
  std::memcpy(buf, s.data(), s.size());
  const int rc = prh_parse_seeds(e, buf, (int64_t)s.size(), n, ids, weights);
  std::free(buf);
  return rc;
}

void good(const prh_edges *e, const std::string &s, int32_t want_n, const int32_t *want_ids, const double *want_w) {
  int32_t n = -1, *ids = nullptr;
  double *w = nullptr;
  const int rc = parse_exact(e, s, &n, &ids, &w);
  expect(rc == 0 && n == want_n, "parse", s);
  for (int32_t i = 0; rc == 0 && i < n && i < want_n; ++i)
    expect(ids[i] == want_ids[i] && w[i] == want_w[i], "seed value", s);
  if (rc == 0) {
    double v[8] = {0};
    if (n <= 8) prh_seed_teleport(n, w, 0.15, prh_n_vertices(e), v);
    double sum = 0.0;
    for (int32_t i = 0; i < n && i < 8; ++i) sum += v[i];
    const double mass = 0.15 * prh_n_vertices(e);
    expect(n > 8 || (sum > mass * (1 - 1e-12) && sum < mass * (1 + 1e-12)), "teleport mass", s);
  }
  prh_free_seeds(ids, w);
}

void bad(const prh_edges *e, const std::string &s, int line) {
  int32_t n = -1, *ids = nullptr;
  double *w = nullptr;
  const int rc = parse_exact(e, s, &n, &ids, &w);
  expect(rc != 0 && n == 0 && !ids && !w, "rejection", s);
  const std::string where = "line " + std::to_string(line) + ":";
  expect(rc != 0 && std::strstr(prh_last_error(), where.c_str()) != nullptr, "line number in the message", s);
  prh_free_seeds(ids, w);
}

}  // namespace

int main() {
  const char edges_txt[] = "A B\nA C\nB C\nC A\nD\n";  // IDs: A 0, B 1, C 2, D 3
  prh_edges *e = nullptr;
  if (prh_parse(edges_txt, (int64_t)sizeof(edges_txt) - 1, PRH_FORMAT_EDGES, &e) != 0) {
    std::fprintf(stderr, "seeds_check: edge list: %s\n", prh_last_error());
    return 1;
  }
  {
    const int32_t ids[] = {2, 0};
    const double w[] = {2.0, 1.0};
    good(e, "C 2\nA\n", 2, ids, w);
    good(e, "C 2\nA", 2, ids, w);  // no final newline
    good(e, "# seeds\n\nC\t2\r\n   \nA 1e0\n", 2, ids, w);
  }
  {
    const int32_t ids[] = {3, 1, 0, 2};
    const double w[] = {0.5, 1.0, 3.0, 1.0};
    good(e, "D 0.5\nB\nA 3\nC\n", 4, ids, w);  // file order
  }
  bad(e, "A\nX 2\n", 2);        // unknown URL
  bad(e, "A\n\n# c\nA 3\n", 4);  // duplicate URL
  bad(e, "A 0\n", 1);
  bad(e, "B\nA -1\n", 2);
  bad(e, "A nan\n", 1);
  bad(e, "A inf\n", 1);
  bad(e, "A -inf\n", 1);
  bad(e, "A 1e999\n", 1);
  bad(e, "A 1x\n", 1);
  bad(e, "A 1 junk\n", 1);  // trailing junk
  bad(e, "A 1 2 3", 1);
  bad(e, "", 1);            // empty file
  bad(e, "\n# only a comment\n", 3);
  // truncated buffers: every prefix of a valid and of a malformed file parses or fails cleanly
  for (const std::string &full : {std::string("C 2.5e-1\nA\nD 7\n"), std::string("# x\nB 1e\nQ 2 3\n")})
    for (size_t len = 0; len <= full.size(); ++len) {
      int32_t n = -1, *ids = nullptr;
      double *w = nullptr;
      const std::string s = full.substr(0, len);
      const int rc = parse_exact(e, s, &n, &ids, &w);
      expect(rc == 0 ? (n >= 1 && ids && w) : (n == 0 && !ids && !w), "prefix outcome", s);
      for (int32_t i = 0; rc == 0 && i < n; ++i)
        expect(ids[i] >= 0 && ids[i] < prh_n_vertices(e) && w[i] > 0.0, "prefix seed in range", s);
      prh_free_seeds(ids, w);
    }
  // bad arguments
  {
    int32_t n = 0, *ids = nullptr;
    double *w = nullptr;
    expect(prh_parse_seeds(nullptr, "A\n", 2, &n, &ids, &w) != 0, "NULL edges", "A");
    expect(prh_parse_seeds(e, nullptr, 2, &n, &ids, &w) != 0, "NULL data", "");
    expect(prh_parse_seeds(e, "A\n", -1, &n, &ids, &w) != 0, "negative len", "A");
    expect(prh_parse_seeds(e, "A\n", 2, nullptr, &ids, &w) != 0, "NULL n", "A");
    expect(prh_read_seeds(e, "/nonexistent/seeds.txt", &n, &ids, &w) != 0, "missing file", "");
    prh_free_seeds(nullptr, nullptr);
  }
  prh_free(e);
  std::printf("seeds_check: done, %d failures\n", g_failures);
  return g_failures == 0 ? 0 : 1;
}
