// Stand-alone driver for gpushare_amd/native/http_parse.h, meant to be built
// with -fsanitize=address,undefined.  Every response in the table is parsed
// whole, split in two at every offset, and one byte at a time; each run must
// give the same status, body and flags (or the same error).  Exit status 0
// and a final "OK" line mean every check held.

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../gpushare_amd/native/http_parse.h"

using httpwire::Error;
using httpwire::Feed;
using httpwire::ResponseParser;

namespace {

int g_failures = 0;

#define CHECK(cond, ...)                                      \
  do {                                                        \
    if (!(cond)) {                                            \
      ++g_failures;                                           \
      std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                      \
      std::fprintf(stderr, "\n");                             \
    }                                                         \
  } while (0)

struct Case {
  std::string name;
  std::string wire;
  bool head_request;
  bool eof_after;  // the peer closes after the last byte
  Error want_error;  // Error::none: a valid response
  int status;
  std::string body;
  bool keep_alive;
  bool exhaustive;  // split at every offset (small cases) or a sample
};

// Feeds the pieces through a heap copy of exactly their size, so a read past
// the end of a piece is a heap-buffer-overflow under AddressSanitizer.
Feed feed_piece(ResponseParser &p, const char *data, size_t n) {
  std::vector<char> copy(data, data + n);
  return p.feed(copy.data(), copy.size());
}

void check_outcome(const Case &c, ResponseParser &p, Feed last,
                   const char *how, size_t at) {
  if (c.eof_after && last == Feed::need_more) last = p.finish_eof();
  if (c.want_error != Error::none) {
    CHECK(last == Feed::error, "%s [%s@%zu]: expected an error", c.name.c_str(),
          how, at);
    CHECK(p.error() == c.want_error, "%s [%s@%zu]: error %d, want %d",
          c.name.c_str(), how, at, static_cast<int>(p.error()),
          static_cast<int>(c.want_error));
    CHECK(!p.done(), "%s [%s@%zu]: done after error", c.name.c_str(), how, at);
    return;
  }
  CHECK(last == Feed::done, "%s [%s@%zu]: not done (error %d)", c.name.c_str(),
        how, at, static_cast<int>(p.error()));
  if (last != Feed::done) return;
  CHECK(p.status() == c.status, "%s [%s@%zu]: status %d, want %d",
        c.name.c_str(), how, at, p.status(), c.status);
  CHECK(p.body() == c.body, "%s [%s@%zu]: body of %zu bytes, want %zu",
        c.name.c_str(), how, at, p.body().size(), c.body.size());
  CHECK(p.keep_alive() == c.keep_alive, "%s [%s@%zu]: keep_alive %d, want %d",
        c.name.c_str(), how, at, p.keep_alive(), c.keep_alive);
  CHECK(p.excess() == 0, "%s [%s@%zu]: excess %zu", c.name.c_str(), how, at,
        p.excess());
}

void run_case(const Case &c) {
  const std::string &w = c.wire;
  ResponseParser p;

  // whole
  p.reset(c.head_request);
  Feed f = feed_piece(p, w.data(), w.size());
  check_outcome(c, p, f, "whole", 0);

  // two pieces, split at every offset (or a sample of them)
  for (size_t cut = 0; cut <= w.size(); ++cut) {
    if (!c.exhaustive && cut > 64 && cut + 64 < w.size() && cut % 65537 != 0)
      continue;
    p.reset(c.head_request);
    f = feed_piece(p, w.data(), cut);
    if (f == Feed::need_more) f = feed_piece(p, w.data() + cut, w.size() - cut);
    check_outcome(c, p, f, "split", cut);
  }

  // one byte at a time; stop at the first verdict
  p.reset(c.head_request);
  f = Feed::need_more;
  size_t i = 0;
  for (; i < w.size() && f == Feed::need_more; ++i)
    f = feed_piece(p, w.data() + i, 1);
  if (c.want_error == Error::none)
    CHECK(i == w.size(), "%s [bytes]: verdict after %zu of %zu bytes",
          c.name.c_str(), i, w.size());
  check_outcome(c, p, f, "bytes", i);
}

Case ok(const char *name, std::string wire, int status, std::string body,
        bool keep_alive, bool eof_after = false, bool head = false,
        bool exhaustive = true) {
  return Case{name, std::move(wire), head, eof_after, Error::none, status,
              std::move(body), keep_alive, exhaustive};
}

Case bad(const char *name, std::string wire, Error e, bool eof_after = false,
         bool exhaustive = true) {
  return Case{name, std::move(wire), false, eof_after, e, 0, "", false,
              exhaustive};
}

void test_parser() {
  std::string big(1 << 20, '\0');
  for (size_t i = 0; i < big.size(); ++i)
    big[i] = static_cast<char>('a' + (i * 7 + i / 251) % 26);
  std::string big_chunked;
  for (size_t off = 0; off < big.size();) {
    size_t n = 1 + (off * 31 + 17) % 70001;
    if (n > big.size() - off) n = big.size() - off;
    char hex[32];
    std::snprintf(hex, sizeof hex, "%zx\r\n", n);
    big_chunked += hex;
    big_chunked.append(big, off, n);
    big_chunked += "\r\n";
    off += n;
  }
  big_chunked += "0\r\n\r\n";

  std::vector<Case> cases = {
      ok("content-length",
         "HTTP/1.1 200 OK\r\nContent-Type: application/json\r\n"
         "Content-Length: 11\r\n\r\n{\"ok\":true}",
         200, "{\"ok\":true}", true),
      ok("empty body", "HTTP/1.1 200 X\r\nContent-Length: 0\r\n\r\n", 200, "",
         true),
      ok("204", "HTTP/1.1 204 No Content\r\n\r\n", 204, "", true),
      ok("304 ignores its length",
         "HTTP/1.1 304 Not Modified\r\nContent-Length: 120\r\n\r\n", 304, "",
         true),
      ok("HEAD ignores its length",
         "HTTP/1.1 200 OK\r\nContent-Length: 120\r\n\r\n", 200, "", true, false,
         true),
      ok("status without reason", "HTTP/1.1 404\r\nContent-Length: 2\r\n\r\nno",
         404, "no", true),
      ok("chunked",
         "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n"
         "5\r\nhello\r\n1\r\n \r\nb\r\nchunked wor\r\n2\r\nld\r\n0\r\n\r\n",
         200, "hello chunked world", true),
      ok("chunk extension and trailer",
         "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n"
         "4;name=value;q=\"x\"\r\nabcd\r\nA ; ext\r\n0123456789\r\n"
         "0;last\r\nX-Checksum: 1234\r\nX-Other: y\r\n\r\n",
         200, "abcd0123456789", true),
      ok("chunked wins over content-length",
         "HTTP/1.1 200 OK\r\nContent-Length: 3\r\n"
         "Transfer-Encoding: gzip, chunked\r\n\r\n2\r\nhi\r\n0\r\n\r\n",
         200, "hi", true),
      ok("header names and values in any case",
         "HTTP/1.1 201 Created\r\ncontent-LENGTH:   3  \r\n"
         "CONNECTION: Keep-Alive\r\n\r\nabc",
         201, "abc", true),
      ok("TRANSFER-ENCODING: Chunked",
         "HTTP/1.1 200 OK\r\nTRANSFER-ENCODING: Chunked\r\n\r\n3\r\nabc\r\n"
         "0\r\n\r\n",
         200, "abc", true),
      ok("100 continue then 200",
         "HTTP/1.1 100 Continue\r\n\r\n"
         "HTTP/1.1 200 OK\r\nContent-Length: 4\r\n\r\ndone",
         200, "done", true),
      ok("100 continue with headers then chunked",
         "HTTP/1.1 100 Continue\r\nX-A: b\r\n\r\n"
         "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n1\r\nz\r\n"
         "0\r\n\r\n",
         200, "z", true),
      ok("connection close",
         "HTTP/1.1 200 OK\r\nConnection: close\r\nContent-Length: 2\r\n\r\nok",
         200, "ok", false),
      ok("connection token list",
         "HTTP/1.1 200 OK\r\nConnection: foo, Close\r\nContent-Length: 2\r\n\r\n"
         "ok",
         200, "ok", false),
      ok("body to end of connection",
         "HTTP/1.1 200 OK\r\nContent-Type: text/plain\r\n\r\nuntil the end\n",
         200, "until the end\n", false, true),
      ok("HTTP/1.0 closes by default",
         "HTTP/1.0 200 OK\r\nContent-Length: 2\r\n\r\nok", 200, "ok", false),
      ok("HTTP/1.0 keep-alive",
         "HTTP/1.0 200 OK\r\nConnection: keep-alive\r\nContent-Length: 2\r\n"
         "\r\nok",
         200, "ok", true),
      ok("bare LF line ends", "HTTP/1.1 200 OK\nContent-Length: 2\n\nok", 200,
         "ok", true),
      ok("1 MiB content-length",
         "HTTP/1.1 200 OK\r\nContent-Length: 1048576\r\n\r\n" + big, 200, big,
         true, false, false, false),
      ok("1 MiB chunked",
         "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n" + big_chunked,
         200, big, true, false, false, false),

      bad("non-numeric chunk size",
          "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\nzz\r\nab\r\n",
          Error::bad_chunk),
      bad("empty chunk size",
          "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n\r\nab\r\n",
          Error::bad_chunk),
      bad("negative chunk size",
          "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n-1\r\nab\r\n",
          Error::bad_chunk),
      bad("overlong chunk size",
          "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n"
          "10000000000000000\r\nab\r\n",
          Error::bad_chunk),
      bad("chunk size of 16 f",
          "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n"
          "ffffffffffffffff\r\nab\r\n",
          Error::bad_chunk),
      bad("chunk size line without end",
          "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n1;" +
              std::string(httpwire::kMaxChunkLine, 'x'),
          Error::bad_chunk),
      bad("chunk data not followed by CRLF",
          "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n2\r\nabXX\r\n",
          Error::bad_chunk),
      bad("negative content-length",
          "HTTP/1.1 200 OK\r\nContent-Length: -5\r\n\r\nhello",
          Error::bad_content_length),
      bad("duplicate content-length",
          "HTTP/1.1 200 OK\r\nContent-Length: 5\r\nContent-Length: 5\r\n\r\n"
          "hello",
          Error::bad_content_length),
      bad("overflowing content-length",
          "HTTP/1.1 200 OK\r\nContent-Length: 18446744073709551621\r\n\r\nhello",
          Error::bad_content_length),
      bad("content-length with junk",
          "HTTP/1.1 200 OK\r\nContent-Length: 5x\r\n\r\nhello",
          Error::bad_content_length),
      bad("empty content-length", "HTTP/1.1 200 OK\r\nContent-Length:\r\n\r\n",
          Error::bad_content_length),
      bad("header block over the cap",
          "HTTP/1.1 200 OK\r\nX-Pad: " +
              std::string(httpwire::kMaxHeadBytes, 'p') +
              "\r\nContent-Length: 0\r\n\r\n",
          Error::head_too_large, false, false),
      bad("many headers over the cap",
          [] {
            std::string s = "HTTP/1.1 200 OK\r\n";
            while (s.size() <= httpwire::kMaxHeadBytes)
              s += "X-Filler-Header: 0123456789abcdef\r\n";
            return s + "\r\n";
          }(),
          Error::head_too_large, false, false),
      bad("header without colon",
          "HTTP/1.1 200 OK\r\nthis is not a header\r\n\r\n", Error::bad_header),
      bad("truncated status line", "HTTP/1.1 20", Error::bad_status_line, true),
      bad("not HTTP", "SSH-2.0-OpenSSH_9.6\r\n", Error::bad_status_line),
      bad("status not a number", "HTTP/1.1 2x0 OK\r\n\r\n",
          Error::bad_status_line),
      bad("status below 100", "HTTP/1.1 099 OK\r\n\r\n",
          Error::bad_status_line),
      bad("four-digit status", "HTTP/1.1 2000 OK\r\n\r\n",
          Error::bad_status_line),
      bad("HTTP/2 preface", "HTTP/2.0 200 OK\r\n\r\n", Error::bad_status_line),
      bad("closed before any byte", "", Error::eof_before_response, true),
      bad("closed inside the head", "HTTP/1.1 200 OK\r\nContent-Le",
          Error::truncated, true),
      bad("closed inside a content-length body",
          "HTTP/1.1 200 OK\r\nContent-Length: 10\r\n\r\nshort", Error::truncated,
          true),
      bad("closed inside a chunk",
          "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n8\r\nabc",
          Error::truncated, true),
      bad("closed before the last chunk",
          "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n3\r\nabc\r\n",
          Error::truncated, true),
  };
  for (const Case &c : cases) run_case(c);
  std::printf("parser: %zu cases\n", cases.size());

  // bytes after the end of a response are counted, not parsed, and make the
  // connection unfit for reuse
  {
    ResponseParser p;
    std::string w = "HTTP/1.1 200 OK\r\nContent-Length: 2\r\n\r\nokHTTP/1.1 5";
    Feed f = feed_piece(p, w.data(), w.size());
    CHECK(f == Feed::done, "excess: not done");
    CHECK(p.body() == "ok", "excess: body");
    CHECK(p.excess() == 10, "excess: %zu", p.excess());
    CHECK(!p.keep_alive(), "excess: still keep-alive");
    p.reset();
    CHECK(p.excess() == 0 && !p.done() && p.body().empty(), "reset");
  }

  // a reader that takes the body out between feeds sees every byte once
  {
    ResponseParser p;
    std::string w =
        "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n"
        "3\r\nab\n\r\n5\r\ncd\nef\r\n0\r\n\r\n";
    std::string seen;
    for (size_t i = 0; i < w.size(); ++i) {
      feed_piece(p, w.data() + i, 1);
      seen += p.body();
      p.body().clear();
    }
    CHECK(p.done() && seen == "ab\ncd\nef", "streaming take-out: '%s'",
          seen.c_str());
  }
}

void test_builder() {
  using httpwire::build_head;
  using httpwire::Headers;
  std::string out, err;

  CHECK(build_head(out, "GET", "/api/v1/pods?watch=true", "127.0.0.1:8080",
                   Headers{{"Accept", "application/json"}}, -1, &err),
        "GET refused: %s", err.c_str());
  CHECK(out ==
            "GET /api/v1/pods?watch=true HTTP/1.1\r\nHost: 127.0.0.1:8080\r\n"
            "Accept-Encoding: identity\r\nAccept: application/json\r\n\r\n",
        "GET head: %s", out.c_str());

  out.clear();
  CHECK(build_head(out, "PATCH", "/p", "h",
                   Headers{{"Accept", "a"}, {"Content-Type", "b"}}, 2, &err),
        "PATCH refused");
  CHECK(out ==
            "PATCH /p HTTP/1.1\r\nHost: h\r\nAccept-Encoding: identity\r\n"
            "Content-Length: 2\r\nAccept: a\r\nContent-Type: b\r\n\r\n",
        "PATCH head: %s", out.c_str());

  out.clear();
  CHECK(build_head(out, "POST", "/p", "h", Headers{}, -1, &err), "POST refused");
  CHECK(out ==
            "POST /p HTTP/1.1\r\nHost: h\r\nAccept-Encoding: identity\r\n"
            "Content-Length: 0\r\n\r\n",
        "body-less POST head: %s", out.c_str());

  out.clear();
  CHECK(build_head(out, "DELETE", "/p", "h", Headers{}, -1, &err), "DELETE");
  CHECK(out == "DELETE /p HTTP/1.1\r\nHost: h\r\nAccept-Encoding: identity\r\n\r\n",
        "DELETE head: %s", out.c_str());

  out.clear();
  CHECK(build_head(out, "GET", "/", "h",
                   Headers{{"host", "other"}, {"ACCEPT-ENCODING", "gzip"},
                           {"content-length", "7"}},
                   3, &err),
        "overrides refused");
  CHECK(out ==
            "GET / HTTP/1.1\r\nhost: other\r\nACCEPT-ENCODING: gzip\r\n"
            "content-length: 7\r\n\r\n",
        "override head: %s", out.c_str());

  struct Rej {
    const char *method, *path, *name, *value;
  } rejects[] = {
      {"GET", "/a\r\nX-Injected: 1", "A", "b"},
      {"GET", "/a\nb", "A", "b"},
      {"GET", "/a b", "A", "b"},
      {"GET", "", "A", "b"},
      {"GE\rT", "/", "A", "b"},
      {"GET", "/", "A\r\nB", "b"},
      {"GET", "/", "A:B", "b"},
      {"GET", "/", "", "b"},
      {"GET", "/", "A", "b\r\nX-Injected: 1"},
      {"GET", "/", "A", "b\nc"},
      {"GET", "/", "A", "b\rc"},
  };
  for (const Rej &r : rejects) {
    out = "untouched";
    err.clear();
    bool okay = build_head(out, r.method, r.path, "h",
                           Headers{{r.name, r.value}}, -1, &err);
    CHECK(!okay && out == "untouched" && !err.empty(),
          "injection accepted: %s %s %s %s", r.method, r.path, r.name, r.value);
  }
  // NUL needs explicit lengths
  out = "untouched";
  CHECK(!build_head(out, "GET", std::string("/a\0b", 4), "h", Headers{}, -1,
                    &err) &&
            out == "untouched",
        "NUL in path accepted");
  CHECK(!build_head(out, "GET", "/", "h",
                    Headers{{"A", std::string("b\0c", 3)}}, -1, &err),
        "NUL in value accepted");

  CHECK(httpwire::host_header("example.org", 80, 80) == "example.org", "host 80");
  CHECK(httpwire::host_header("example.org", 443, 443) == "example.org",
        "host 443");
  CHECK(httpwire::host_header("127.0.0.1", 8080, 80) == "127.0.0.1:8080",
        "host port");
  CHECK(httpwire::host_header("::1", 8080, 80) == "[::1]:8080", "host v6");
  std::printf("builder: checked\n");
}

}  // namespace

int main() {
  test_parser();
  test_builder();
  if (g_failures) {
    std::fprintf(stderr, "%d check(s) failed\n", g_failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
