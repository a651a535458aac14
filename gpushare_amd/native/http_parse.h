// HTTP/1.1 client wire format: request-head builder and incremental response
// parser.  No Python, no sockets, no allocation beyond std::string — the
// extension (http_rt.cpp) and the stand-alone sanitizer driver
// (tests/native/http_parse_driver.cpp) both include this file as is.
//
// The builder emits byte for byte what stdlib http.client emits for
// conn.request(method, path, body, headers):
//
//   METHOD path HTTP/1.1
//   Host: host[:port]            (unless the caller passes Host)
//   Accept-Encoding: identity    (unless the caller passes Accept-Encoding)
//   Content-Length: n            (unless the caller passes Content-Length or
//                                 Transfer-Encoding; only with a body, or as
//                                 0 for a body-less POST/PUT/PATCH)
//   caller's headers, in order
//
// The parser is fed whatever recv() returned, in pieces of any size, and
// never reads past the end of the piece it was given.

#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace httpwire {

using Headers = std::vector<std::pair<std::string, std::string>>;

constexpr size_t kMaxHeadBytes = 64 * 1024;  // status line + headers + trailers
constexpr size_t kMaxChunkLine = 4 * 1024;   // chunk size + extensions
constexpr int kMaxChunkDigits = 15;          // 60 bits: cannot wrap int64/size_t

inline char lower(char c) {
  return (c >= 'A' && c <= 'Z') ? static_cast<char>(c + 32) : c;
}

inline bool iequals(const char *a, size_t an, const char *lit) {
  size_t i = 0;
  for (; i < an && lit[i]; ++i)
    if (lower(a[i]) != lit[i]) return false;
  return i == an && lit[i] == '\0';
}

// "host", "host:port" or "[v6]:port"; the port is left out when it is the
// scheme's default, as http.client does.
inline std::string host_header(const std::string &host, int port,
                               int default_port) {
  std::string out;
  if (host.find(':') != std::string::npos) {
    out = "[" + host + "]";
  } else {
    out = host;
  }
  if (port != default_port) out += ":" + std::to_string(port);
  return out;
}

inline bool has_ctl(const std::string &s, bool reject_space) {
  for (unsigned char c : s) {
    if (c == '\r' || c == '\n' || c == '\0') return true;
    if (reject_space && (c <= 0x20 || c == 0x7f)) return true;
  }
  return false;
}

// Appends the request head (through the blank line) to `out`.  body_len < 0
// means "no body given".  Returns false, with a reason in *err and `out`
// untouched, if any part could smuggle a line break into the head.
inline bool build_head(std::string &out, const std::string &method,
                       const std::string &path, const std::string &host,
                       const Headers &headers, int64_t body_len,
                       std::string *err) {
  auto fail = [&](const char *what) {
    if (err) *err = what;
    return false;
  };
  if (method.empty() || has_ctl(method, true))
    return fail("method contains control characters or spaces");
  if (path.empty() || has_ctl(path, true))
    return fail("path contains control characters or spaces");
  if (has_ctl(host, true)) return fail("host contains control characters");
  bool has_host = false, has_ae = false, has_cl = false, has_te = false;
  for (const auto &h : headers) {
    const std::string &n = h.first;
    if (n.empty() || has_ctl(n, true) || n.find(':') != std::string::npos)
      return fail("invalid header name");
    if (has_ctl(h.second, false)) return fail("invalid header value");
    if (iequals(n.data(), n.size(), "host")) has_host = true;
    if (iequals(n.data(), n.size(), "accept-encoding")) has_ae = true;
    if (iequals(n.data(), n.size(), "content-length")) has_cl = true;
    if (iequals(n.data(), n.size(), "transfer-encoding")) has_te = true;
  }

  std::string head;
  head.reserve(256);
  head += method;
  head += ' ';
  head += path;
  head += " HTTP/1.1\r\n";
  if (!has_host) {
    head += "Host: ";
    head += host;
    head += "\r\n";
  }
  if (!has_ae) head += "Accept-Encoding: identity\r\n";
  if (!has_cl && !has_te) {
    int64_t n = body_len;
    if (n < 0) {
      std::string m;
      for (char c : method) m += lower(c);
      if (m == "post" || m == "put" || m == "patch") n = 0;
    }
    if (n >= 0) {
      head += "Content-Length: ";
      head += std::to_string(n);
      head += "\r\n";
    }
  }
  for (const auto &h : headers) {
    head += h.first;
    head += ": ";
    head += h.second;
    head += "\r\n";
  }
  head += "\r\n";
  out += head;
  return true;
}

enum class Feed { need_more, done, error };

enum class Error {
  none,
  eof_before_response,  // peer closed before the first response byte
  bad_status_line,
  head_too_large,
  bad_header,
  bad_content_length,
  bad_chunk,
  truncated,  // peer closed inside the head or inside a framed body
};

class ResponseParser {
 public:
  explicit ResponseParser(bool head_request = false) { reset(head_request); }

  void reset(bool head_request = false) {
    head_request_ = head_request;
    state_ = State::status_line;
    error_ = Error::none;
    line_.clear();
    body_.clear();
    head_bytes_ = 0;
    any_bytes_ = false;
    status_ = 0;
    minor_ = 1;
    begin_message();
    excess_ = 0;
  }

  // Consumes at most n bytes; bytes after the end of the response are not
  // touched and are counted in excess().
  Feed feed(const char *p, size_t n) {
    if (state_ == State::failed) return Feed::error;
    if (state_ == State::done) {
      excess_ += n;
      return Feed::done;
    }
    if (n) any_bytes_ = true;
    size_t i = 0;
    while (i < n) {
      switch (state_) {
        case State::status_line:
        case State::headers:
        case State::chunk_size:
        case State::chunk_crlf:
        case State::trailers: {
          // line-oriented states: gather up to and including '\n'
          const char *nl =
              static_cast<const char *>(std::memchr(p + i, '\n', n - i));
          size_t take = nl ? static_cast<size_t>(nl - (p + i)) + 1 : n - i;
          // chunk lines are capped each; head and trailer lines share one
          // budget.  used <= cap always holds, so the subtraction is safe.
          bool chunk_line =
              state_ == State::chunk_size || state_ == State::chunk_crlf;
          size_t cap = chunk_line ? kMaxChunkLine : kMaxHeadBytes;
          size_t used = chunk_line ? line_.size() : head_bytes_;
          if (take > cap - used)
            return fail(chunk_line ? Error::bad_chunk : Error::head_too_large);
          line_.append(p + i, take);
          if (!chunk_line) head_bytes_ += take;
          i += take;
          if (!nl) break;
          // strip LF and an optional CR
          line_.pop_back();
          if (!line_.empty() && line_.back() == '\r') line_.pop_back();
          if (!on_line()) return Feed::error;
          line_.clear();
          break;
        }
        case State::body_length: {
          uint64_t want = remaining_;
          size_t take = (n - i) < want ? (n - i) : static_cast<size_t>(want);
          body_.append(p + i, take);
          i += take;
          remaining_ -= take;
          if (remaining_ == 0) state_ = State::done;
          break;
        }
        case State::chunk_data: {
          uint64_t want = remaining_;
          size_t take = (n - i) < want ? (n - i) : static_cast<size_t>(want);
          body_.append(p + i, take);
          i += take;
          remaining_ -= take;
          if (remaining_ == 0) state_ = State::chunk_crlf;
          break;
        }
        case State::body_eof:
          body_.append(p + i, n - i);
          i = n;
          break;
        case State::done:
          excess_ += n - i;
          i = n;
          break;
        case State::failed:
          return Feed::error;
      }
    }
    if (state_ == State::done) return Feed::done;
    return Feed::need_more;
  }

  // The peer closed the connection.
  Feed finish_eof() {
    switch (state_) {
      case State::done:
        return Feed::done;
      case State::failed:
        return Feed::error;
      case State::body_eof:
        state_ = State::done;
        return Feed::done;
      case State::status_line:
        if (!any_bytes_) return fail(Error::eof_before_response);
        return fail(Error::bad_status_line);
      default:
        return fail(Error::truncated);
    }
  }

  Error error() const { return error_; }
  bool done() const { return state_ == State::done; }
  bool any_bytes() const { return any_bytes_; }
  // true once the status line and all headers of the final response are in
  bool head_complete() const {
    switch (state_) {
      case State::status_line:
      case State::headers:
      case State::failed:
        return false;
      default:
        return true;
    }
  }
  int status() const { return status_; }
  // De-framed body bytes received so far.  A streaming reader may take them
  // out between feeds (std::string::swap / clear): the parser only appends.
  std::string &body() { return body_; }
  const std::string &body() const { return body_; }
  // Valid once done(): may another request go out on this connection?
  bool keep_alive() const {
    return state_ == State::done && keep_alive_ && !eof_body_ && excess_ == 0;
  }
  size_t excess() const { return excess_; }

 private:
  enum class State {
    status_line,
    headers,
    body_length,
    body_eof,
    chunk_size,
    chunk_data,
    chunk_crlf,
    trailers,
    done,
    failed,
  };

  Feed fail(Error e) {
    error_ = e;
    state_ = State::failed;
    return Feed::error;
  }

  void begin_message() {
    chunked_ = false;
    have_length_ = false;
    length_ = 0;
    remaining_ = 0;
    conn_close_ = false;
    conn_keep_alive_ = false;
    keep_alive_ = false;
    eof_body_ = false;
  }

  bool on_line() {
    switch (state_) {
      case State::status_line:
        return on_status_line();
      case State::headers:
        if (line_.empty()) return on_head_end();
        return on_header();
      case State::chunk_size:
        return on_chunk_size();
      case State::chunk_crlf:
        if (!line_.empty()) {
          fail(Error::bad_chunk);
          return false;
        }
        state_ = State::chunk_size;
        return true;
      case State::trailers:
        if (line_.empty()) state_ = State::done;
        return true;
      default:
        return true;
    }
  }

  // "HTTP/1.x SSS[ reason]"
  bool on_status_line() {
    const std::string &l = line_;
    if (l.size() < 12 || l.compare(0, 7, "HTTP/1.") != 0 ||
        (l[7] != '0' && l[7] != '1') || l[8] != ' ') {
      fail(Error::bad_status_line);
      return false;
    }
    int code = 0;
    for (int k = 9; k < 12; ++k) {
      if (l[k] < '0' || l[k] > '9') {
        fail(Error::bad_status_line);
        return false;
      }
      code = code * 10 + (l[k] - '0');
    }
    if (code < 100 || (l.size() > 12 && l[12] != ' ')) {
      fail(Error::bad_status_line);
      return false;
    }
    minor_ = l[7] - '0';
    status_ = code;
    begin_message();
    state_ = State::headers;
    return true;
  }

  bool on_header() {
    const std::string &l = line_;
    if (l[0] == ' ' || l[0] == '\t') return true;  // obsolete folding: ignore
    size_t colon = l.find(':');
    if (colon == std::string::npos || colon == 0) {
      fail(Error::bad_header);
      return false;
    }
    size_t ne = colon;
    while (ne > 0 && (l[ne - 1] == ' ' || l[ne - 1] == '\t')) --ne;
    size_t vb = colon + 1, ve = l.size();
    while (vb < ve && (l[vb] == ' ' || l[vb] == '\t')) ++vb;
    while (ve > vb && (l[ve - 1] == ' ' || l[ve - 1] == '\t')) --ve;
    const char *name = l.data();
    const char *val = l.data() + vb;
    size_t vn = ve - vb;
    if (iequals(name, ne, "content-length")) {
      if (have_length_ || vn == 0 || vn > 18) {  // 18 digits < 2^63
        fail(Error::bad_content_length);
        return false;
      }
      uint64_t v = 0;
      for (size_t k = 0; k < vn; ++k) {
        if (val[k] < '0' || val[k] > '9') {
          fail(Error::bad_content_length);
          return false;
        }
        v = v * 10 + static_cast<uint64_t>(val[k] - '0');
      }
      have_length_ = true;
      length_ = v;
    } else if (iequals(name, ne, "transfer-encoding")) {
      if (has_token(val, vn, "chunked")) chunked_ = true;
    } else if (iequals(name, ne, "connection")) {
      if (has_token(val, vn, "close")) conn_close_ = true;
      if (has_token(val, vn, "keep-alive")) conn_keep_alive_ = true;
    }
    return true;
  }

  // comma-separated, case-insensitive token list
  static bool has_token(const char *v, size_t n, const char *tok) {
    size_t i = 0;
    while (i < n) {
      while (i < n && (v[i] == ' ' || v[i] == '\t' || v[i] == ',')) ++i;
      size_t b = i;
      while (i < n && v[i] != ',') ++i;
      size_t e = i;
      while (e > b && (v[e - 1] == ' ' || v[e - 1] == '\t')) --e;
      if (iequals(v + b, e - b, tok)) return true;
    }
    return false;
  }

  bool on_head_end() {
    if (status_ == 100) {  // interim: the real response follows
      state_ = State::status_line;
      return true;
    }
    keep_alive_ = minor_ >= 1 ? !conn_close_ : (conn_keep_alive_ && !conn_close_);
    bool bodyless = head_request_ || (status_ >= 100 && status_ < 200) ||
                    status_ == 204 || status_ == 304;
    if (bodyless) {
      state_ = State::done;
    } else if (chunked_) {
      state_ = State::chunk_size;
    } else if (have_length_) {
      remaining_ = length_;
      state_ = length_ == 0 ? State::done : State::body_length;
    } else {
      eof_body_ = true;
      state_ = State::body_eof;
    }
    return true;
  }

  // hex size, then optional whitespace and ";extensions"
  bool on_chunk_size() {
    const std::string &l = line_;
    uint64_t v = 0;
    int digits = 0;
    size_t k = 0;
    for (; k < l.size(); ++k) {
      char c = l[k];
      int d;
      if (c >= '0' && c <= '9') d = c - '0';
      else if (c >= 'a' && c <= 'f') d = c - 'a' + 10;
      else if (c >= 'A' && c <= 'F') d = c - 'A' + 10;
      else break;
      if (++digits > kMaxChunkDigits) {
        fail(Error::bad_chunk);
        return false;
      }
      v = (v << 4) | static_cast<uint64_t>(d);
    }
    while (k < l.size() && (l[k] == ' ' || l[k] == '\t')) ++k;
    if (digits == 0 || (k < l.size() && l[k] != ';')) {
      fail(Error::bad_chunk);
      return false;
    }
    if (v == 0) {
      state_ = State::trailers;
    } else {
      remaining_ = v;
      state_ = State::chunk_data;
    }
    return true;
  }

  bool head_request_ = false;
  State state_ = State::status_line;
  Error error_ = Error::none;
  std::string line_;
  std::string body_;
  size_t head_bytes_ = 0;
  bool any_bytes_ = false;
  int status_ = 0;
  int minor_ = 1;
  bool chunked_ = false, have_length_ = false;
  uint64_t length_ = 0, remaining_ = 0;
  bool conn_close_ = false, conn_keep_alive_ = false, keep_alive_ = false;
  bool eof_body_ = false;
  size_t excess_ = 0;
};

}  // namespace httpwire
