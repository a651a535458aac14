// gpushare_amd._httprt — keep-alive HTTP/1.1 client round trips without the
// interpreter in the loop.
//
// Every control-plane REST hop (extender filter/bind, the ASSIGNED patch
// inside Allocate, pod create/delete) is a sub-KiB request and a sub-KiB
// response on a pooled connection.  On stdlib http.client about three
// quarters of such a hop is Python: putrequest/putheader, email.parser on
// the response headers, HTTPResponse construction.  Here the head is
// assembled, written together with the body in one sendmsg, and the response
// is received and parsed with the GIL released, so a gRPC worker in the
// middle of its PATCH does not hold up the informer thread (or the other way
// round).  Wire format and framing rules live in http_parse.h.
//
//   Conn           one pooled plain-TCP connection: roundtrip() -> (status, body)
//   LineStream     long-lived GET (k8s watch): readline() de-chunks
//   ResponseParser / build_head   the same parser and builder for callers
//                  that own the socket themselves (TLS through ssl.SSLSocket)
//
// Exceptions are the ones http.client raises for the same condition, because
// HttpSession's stale-connection retry is keyed on them.

#include <pybind11/pybind11.h>

#include <arpa/inet.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <sys/socket.h>
#include <sys/types.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "http_parse.h"

namespace py = pybind11;
using httpwire::Error;
using httpwire::Feed;
using httpwire::Headers;
using httpwire::ResponseParser;

namespace {

// ---- exception classes (looked up once, never released) -------------------
PyObject *g_RemoteDisconnected, *g_BadStatusLine, *g_IncompleteRead,
    *g_LineTooLong, *g_HTTPException, *g_gaierror;

// ---- GIL ------------------------------------------------------------------
// A daemon thread that comes back from a blocking wait while the interpreter
// shuts down must not touch it again.  Before 3.13 PyEval_RestoreThread
// answers that with pthread_exit(), whose forced unwind through C++ frames
// aborts the process; parking the thread (what 3.14 does itself) lets the
// interpreter finish and the process exit normally.
inline bool finalizing() {
#if PY_VERSION_HEX >= 0x030D0000
  return Py_IsFinalizing() != 0;
#else
  return _Py_IsFinalizing() != 0;
#endif
}

inline void reacquire(PyThreadState *ts) {
  if (finalizing())
    for (;;) pause();
  PyEval_RestoreThread(ts);
}

// ---- socket ---------------------------------------------------------------
enum class Rc {
  ok,
  timeout,
  intr,       // a signal arrived: let Python run its handlers, then resume
  os_error,   // err holds errno
  gai_error,  // err holds the getaddrinfo code
  eof_early,  // peer closed before the first response byte
  parse,      // the parser holds the reason
};

struct Io {
  Rc rc = Rc::ok;
  int err = 0;
  explicit operator bool() const { return rc == Rc::ok; }
};

inline Io io_errno() { return Io{Rc::os_error, errno}; }

using Clock = std::chrono::steady_clock;

class Sock {
 public:
  Sock() = default;
  Sock(const Sock &) = delete;
  Sock &operator=(const Sock &) = delete;
  ~Sock() { close(); }

  int fd() const { return fd_; }
  bool is_open() const { return fd_ >= 0; }
  void set_timeout(double s) { timeout_s_ = s; }

  void close() {
    if (fd_ >= 0) {
      ::close(fd_);
      fd_ = -1;
    }
  }
  void shutdown() {
    if (fd_ >= 0) ::shutdown(fd_, SHUT_RDWR);
  }

  // One blocking wait, at most timeout_s_ long (negative: no limit).
  Io wait(short events) const {
    struct pollfd p = {fd_, events, 0};
    int ms = -1;
    if (timeout_s_ >= 0) {
      double v = timeout_s_ * 1e3;
      ms = v > 2147483000.0 ? 2147483000 : static_cast<int>(v + 0.999);
    }
    int r = ::poll(&p, 1, ms);
    if (r > 0) return Io{};
    if (r == 0) return Io{Rc::timeout, 0};
    if (errno == EINTR) return Io{Rc::intr, 0};
    return io_errno();
  }

  // Resolve and connect; tries each address in turn like
  // socket.create_connection and reports the last failure.
  Io connect(const std::string &host, int port) {
    struct addrinfo hints;
    std::memset(&hints, 0, sizeof hints);
    hints.ai_family = AF_UNSPEC;
    hints.ai_socktype = SOCK_STREAM;
    struct addrinfo *res = nullptr;
    std::string service = std::to_string(port);
    int g = ::getaddrinfo(host.c_str(), service.c_str(), &hints, &res);
    if (g != 0) return Io{Rc::gai_error, g};
    Io last{Rc::os_error, ECONNREFUSED};
    for (struct addrinfo *ai = res; ai; ai = ai->ai_next) {
      int fd = ::socket(ai->ai_family,
                        ai->ai_socktype | SOCK_NONBLOCK | SOCK_CLOEXEC,
                        ai->ai_protocol);
      if (fd < 0) {
        last = io_errno();
        continue;
      }
      fd_ = fd;
      last = connect_one(ai);
      if (last) break;
      close();
    }
    ::freeaddrinfo(res);
    if (last) {
      int one = 1;
      ::setsockopt(fd_, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
    }
    return last;
  }

 private:
  Io connect_one(const struct addrinfo *ai) {
    if (::connect(fd_, ai->ai_addr, ai->ai_addrlen) == 0) return Io{};
    if (errno != EINPROGRESS && errno != EINTR) return io_errno();
    // the connect goes on in the background; a signal only restarts the wait
    auto deadline = Clock::now() + std::chrono::duration<double>(
                                       timeout_s_ >= 0 ? timeout_s_ : 0.0);
    for (;;) {
      struct pollfd p = {fd_, POLLOUT, 0};
      int ms = -1;
      if (timeout_s_ >= 0) {
        auto left = std::chrono::duration_cast<std::chrono::milliseconds>(
                        deadline - Clock::now())
                        .count();
        if (left < 0) left = 0;
        ms = left > 2147483000 ? 2147483000 : static_cast<int>(left) + 1;
      }
      int r = ::poll(&p, 1, ms);
      if (r == 0) return Io{Rc::timeout, 0};
      if (r < 0) {
        if (errno == EINTR) continue;
        return io_errno();
      }
      break;
    }
    int soerr = 0;
    socklen_t len = sizeof soerr;
    if (::getsockopt(fd_, SOL_SOCKET, SO_ERROR, &soerr, &len) < 0)
      return io_errno();
    if (soerr != 0) return Io{Rc::os_error, soerr};
    return Io{};
  }

  int fd_ = -1;
  double timeout_s_ = -1.0;
};

// Write head then body, resuming at *off after a short write or a signal.
// sendmsg is writev with MSG_NOSIGNAL: a dead peer gives EPIPE, not SIGPIPE.
Io send_all(const Sock &s, const char *head, size_t head_n, const char *body,
            size_t body_n, size_t *off) {
  const size_t total = head_n + body_n;
  while (*off < total) {
    struct iovec iov[2];
    int cnt = 0;
    if (*off < head_n) {
      iov[cnt].iov_base = const_cast<char *>(head + *off);
      iov[cnt].iov_len = head_n - *off;
      ++cnt;
      if (body_n) {
        iov[cnt].iov_base = const_cast<char *>(body);
        iov[cnt].iov_len = body_n;
        ++cnt;
      }
    } else {
      size_t boff = *off - head_n;
      iov[cnt].iov_base = const_cast<char *>(body + boff);
      iov[cnt].iov_len = body_n - boff;
      ++cnt;
    }
    struct msghdr msg;
    std::memset(&msg, 0, sizeof msg);
    msg.msg_iov = iov;
    msg.msg_iovlen = cnt;
    ssize_t w = ::sendmsg(s.fd(), &msg, MSG_NOSIGNAL);
    if (w >= 0) {
      *off += static_cast<size_t>(w);
      continue;
    }
    if (errno == EINTR) continue;
    if (errno == EAGAIN || errno == EWOULDBLOCK) {
      Io wres = s.wait(POLLOUT);
      if (!wres) return wres;
      continue;
    }
    return io_errno();
  }
  return Io{};
}

// Wait for, receive and parse one piece.  *eof is set when the peer closed.
Io recv_some(const Sock &s, std::vector<char> &buf, ResponseParser &parser,
             bool *eof) {
  for (;;) {
    Io wres = s.wait(POLLIN);
    if (!wres) return wres;
    ssize_t n = ::recv(s.fd(), buf.data(), buf.size(), 0);
    if (n > 0) {
      if (parser.feed(buf.data(), static_cast<size_t>(n)) == Feed::error)
        return Io{Rc::parse, 0};
      return Io{};
    }
    if (n == 0) {
      *eof = true;
      return Io{};
    }
    if (errno == EINTR || errno == EAGAIN || errno == EWOULDBLOCK) continue;
    return io_errno();
  }
}

// ---- Python <-> bytes -----------------------------------------------------
// Request-line parts are ASCII, header parts latin-1, as in http.client; a
// character outside raises UnicodeEncodeError, which is a ValueError.
std::string to_wire(py::handle h, bool ascii_only) {
  PyObject *o = h.ptr();
  if (PyUnicode_Check(o)) {
    if (PyUnicode_IS_ASCII(o)) {
      Py_ssize_t n = 0;
      const char *p = PyUnicode_AsUTF8AndSize(o, &n);
      if (!p) throw py::error_already_set();
      return std::string(p, static_cast<size_t>(n));
    }
    PyObject *b = ascii_only ? PyUnicode_AsASCIIString(o)
                             : PyUnicode_AsLatin1String(o);
    if (!b) throw py::error_already_set();
    std::string out(PyBytes_AS_STRING(b),
                    static_cast<size_t>(PyBytes_GET_SIZE(b)));
    Py_DECREF(b);
    return out;
  }
  if (PyBytes_Check(o))
    return std::string(PyBytes_AS_STRING(o),
                       static_cast<size_t>(PyBytes_GET_SIZE(o)));
  if (PyLong_Check(o)) return py::str(h).cast<std::string>();
  throw py::type_error("expected str, bytes or int");
}

Headers to_headers(py::handle h) {
  Headers out;
  if (h.is_none()) return out;
  if (PyDict_Check(h.ptr())) {
    PyObject *k, *v;
    Py_ssize_t pos = 0;
    while (PyDict_Next(h.ptr(), &pos, &k, &v))
      out.emplace_back(to_wire(k, false), to_wire(v, false));
    return out;
  }
  for (py::handle item : h) {
    py::sequence pair = py::reinterpret_borrow<py::sequence>(item);
    if (py::len(pair) != 2) throw py::value_error("header is not a pair");
    out.emplace_back(to_wire(pair[0], false), to_wire(pair[1], false));
  }
  return out;
}

std::string make_head(py::handle method, py::handle path,
                      const std::string &host, py::handle headers,
                      int64_t body_len) {
  std::string head, err;
  if (!httpwire::build_head(head, to_wire(method, true), to_wire(path, true),
                            host, to_headers(headers), body_len, &err))
    throw py::value_error(err);
  return head;
}

// ---- raising --------------------------------------------------------------
[[noreturn]] void raise_obj(PyObject *type, PyObject *args) {
  PyErr_SetObject(type, args);
  Py_XDECREF(args);
  throw py::error_already_set();
}

[[noreturn]] void raise_parse(const ResponseParser &p) {
  switch (p.error()) {
    case Error::eof_before_response:
      raise_obj(g_RemoteDisconnected,
                Py_BuildValue("(s)",
                              "Remote end closed connection without response"));
    case Error::bad_status_line:
      raise_obj(g_BadStatusLine, Py_BuildValue("(s)", "malformed status line"));
    case Error::head_too_large:
      raise_obj(g_LineTooLong, Py_BuildValue("(s)", "header block"));
    case Error::truncated:
      raise_obj(g_IncompleteRead,
                Py_BuildValue("(N)", PyBytes_FromStringAndSize(
                                         p.body().data(),
                                         static_cast<Py_ssize_t>(
                                             p.body().size()))));
    case Error::bad_header:
      raise_obj(g_HTTPException, Py_BuildValue("(s)", "malformed header line"));
    case Error::bad_content_length:
      raise_obj(g_HTTPException,
                Py_BuildValue("(s)", "invalid Content-Length"));
    case Error::bad_chunk:
      raise_obj(g_HTTPException, Py_BuildValue("(s)", "invalid chunk framing"));
    case Error::none:
      break;
  }
  raise_obj(g_HTTPException, Py_BuildValue("(s)", "response parse error"));
}

[[noreturn]] void raise_io(Io io, const ResponseParser *p) {
  switch (io.rc) {
    case Rc::timeout:
      PyErr_SetString(PyExc_TimeoutError, "timed out");
      throw py::error_already_set();
    case Rc::os_error:
      // OSError picks the subclass from errno: BrokenPipeError,
      // ConnectionResetError, ConnectionRefusedError, ...
      errno = io.err;
      PyErr_SetFromErrno(PyExc_OSError);
      throw py::error_already_set();
    case Rc::gai_error:
      raise_obj(g_gaierror, Py_BuildValue("(is)", io.err, gai_strerror(io.err)));
    case Rc::eof_early:
      raise_obj(g_RemoteDisconnected,
                Py_BuildValue("(s)",
                              "Remote end closed connection without response"));
    case Rc::parse:
      if (p) raise_parse(*p);
      break;
    case Rc::intr:
    case Rc::ok:
      break;
  }
  PyErr_SetString(PyExc_RuntimeError, "httprt: internal error");
  throw py::error_already_set();
}

double timeout_arg(py::handle t) {
  if (t.is_none()) return -1.0;
  double v = t.cast<double>();
  if (v < 0) throw py::value_error("timeout must be non-negative or None");
  return v;
}

// Runs step() with the GIL released until it is done; a signal brings it
// back so Python-level handlers (KeyboardInterrupt) run, then it resumes.
template <typename Step>
Io run_unlocked(Step step) {
  for (;;) {
    PyThreadState *ts = PyEval_SaveThread();
    Io io;
    try {
      io = step();
    } catch (...) {  // std::bad_alloc from a buffer
      io = Io{Rc::os_error, ENOMEM};
    }
    reacquire(ts);
    if (io.rc != Rc::intr) return io;
    if (PyErr_CheckSignals() != 0) throw py::error_already_set();
  }
}

// One user at a time.  Taken and dropped with the GIL held, so a plain flag
// is enough; close() from another thread only wakes the user, who then
// closes the descriptor himself — it is never closed under a running call.
class Busy {
 public:
  Busy(bool &flag, Sock &sock, bool &close_pending)
      : flag_(flag), sock_(sock), close_pending_(close_pending) {
    if (flag_) {
      PyErr_SetString(PyExc_RuntimeError,
                      "connection is in use by another thread");
      throw py::error_already_set();
    }
    flag_ = true;
  }
  ~Busy() {
    flag_ = false;
    if (close_pending_) {
      sock_.close();
      close_pending_ = false;
    }
  }

 private:
  bool &flag_;
  Sock &sock_;
  bool &close_pending_;
};

constexpr size_t kRecvBuf = 64 * 1024;

// ---- Conn -----------------------------------------------------------------
class Conn {
 public:
  Conn(const std::string &host, int port, py::object timeout_s)
      : host_hdr_(httpwire::host_header(host, port, 80)), rbuf_(kRecvBuf) {
    sock_.set_timeout(timeout_arg(timeout_s));
    Io io = run_unlocked([&] { return sock_.connect(host, port); });
    if (!io) {
      sock_.close();
      raise_io(io, nullptr);
    }
  }

  py::tuple roundtrip(py::object method, py::object path, py::object headers,
                      py::object body) {
    if (!sock_.is_open() || close_pending_) {
      PyErr_SetString(PyExc_RuntimeError, "connection closed");
      throw py::error_already_set();
    }
    Busy busy(busy_, sock_, close_pending_);

    // arguments in: the head is assembled here; a bytes body is borrowed
    // (the caller's reference keeps it alive), any other buffer is copied
    const char *body_p = nullptr;
    size_t body_n = 0;
    std::string body_copy;
    int64_t body_len = -1;
    if (!body.is_none()) {
      if (PyBytes_Check(body.ptr())) {
        body_p = PyBytes_AS_STRING(body.ptr());
        body_n = static_cast<size_t>(PyBytes_GET_SIZE(body.ptr()));
      } else {
        py::buffer_info info = py::reinterpret_borrow<py::buffer>(body).request();
        if (info.ndim > 1) throw py::type_error("body must be bytes-like");
        body_copy.assign(static_cast<const char *>(info.ptr),
                         static_cast<size_t>(info.size * info.itemsize));
        body_p = body_copy.data();
        body_n = body_copy.size();
      }
      body_len = static_cast<int64_t>(body_n);
    }
    bool is_head = false;
    {
      std::string m = to_wire(method, true);
      is_head = httpwire::iequals(m.data(), m.size(), "head");
    }
    std::string head = make_head(method, path, host_hdr_, headers, body_len);

    parser_.reset(is_head);
    keep_alive_ = false;
    size_t off = 0;
    bool sent = false, eof = false;
    Io io = run_unlocked([&]() -> Io {
      if (!sent) {
        Io s = send_all(sock_, head.data(), head.size(), body_p, body_n, &off);
        if (!s) return s;
        sent = true;
      }
      while (!parser_.done()) {
        Io r = recv_some(sock_, rbuf_, parser_, &eof);
        if (!r) return r;
        if (eof) {
          if (parser_.finish_eof() == Feed::done) break;
          return Io{parser_.error() == Error::eof_before_response
                        ? Rc::eof_early
                        : Rc::parse,
                    0};
        }
      }
      return Io{};
    });
    if (!io) {
      sock_.close();
      raise_io(io, &parser_);
    }

    // results out
    keep_alive_ = parser_.keep_alive();
    if (!keep_alive_) sock_.close();
    py::bytes data(parser_.body().data(), parser_.body().size());
    if (parser_.body().capacity() > (1u << 20)) std::string().swap(parser_.body());
    return py::make_tuple(parser_.status(), std::move(data));
  }

  void close() {
    if (busy_) {
      close_pending_ = true;
      sock_.shutdown();
    } else {
      sock_.close();
    }
  }

  bool closed() const { return !sock_.is_open(); }
  bool keep_alive() const { return keep_alive_; }
  int fileno() const { return sock_.fd(); }

 private:
  Sock sock_;
  std::string host_hdr_;
  ResponseParser parser_;
  std::vector<char> rbuf_;
  bool keep_alive_ = false;
  bool busy_ = false;
  bool close_pending_ = false;
};

// ---- LineStream -----------------------------------------------------------
class LineStream {
 public:
  LineStream(const std::string &host, int port, py::object timeout_s,
             py::object path, py::object headers, py::object method)
      : rbuf_(kRecvBuf) {
    sock_.set_timeout(timeout_arg(timeout_s));
    std::string m = to_wire(method, true);
    parser_.reset(httpwire::iequals(m.data(), m.size(), "head"));
    std::string head = make_head(method, path,
                                 httpwire::host_header(host, port, 80),
                                 headers, -1);
    bool connected = false, sent = false;
    size_t off = 0;
    Io io = run_unlocked([&]() -> Io {
      if (!connected) {
        Io c = sock_.connect(host, port);
        if (!c) return c;
        connected = true;
      }
      if (!sent) {
        Io s = send_all(sock_, head.data(), head.size(), nullptr, 0, &off);
        if (!s) return s;
        sent = true;
      }
      while (!parser_.head_complete()) {
        Io r = fill();
        if (!r) return r;
        if (eof_ && !parser_.head_complete()) {
          return Io{parser_.error() == Error::eof_before_response
                        ? Rc::eof_early
                        : Rc::parse,
                    0};
        }
      }
      return Io{};
    });
    if (!io) {
      sock_.close();
      raise_io(io, &parser_);
    }
  }

  int status() const { return parser_.status(); }

  // One '\n'-terminated line; the unterminated rest at the end of the
  // stream; then b"".
  py::bytes readline() {
    Busy busy(busy_, sock_, close_pending_);
    size_t nl = std::string::npos;
    Io io = run_unlocked([&]() -> Io {
      for (;;) {
        nl = buf_.find('\n', scan_);
        if (nl != std::string::npos || eof_) return Io{};
        scan_ = buf_.size();
        if (!sock_.is_open()) {
          eof_ = true;
          return Io{};
        }
        Io r = fill();
        if (!r) return r;
      }
    });
    if (!io) {
      sock_.close();
      raise_io(io, &parser_);
    }
    size_t end = nl == std::string::npos ? buf_.size() : nl + 1;
    py::bytes line(buf_.data() + pos_, end - pos_);
    consume(end);
    return line;
  }

  // Everything up to the end of the response.
  py::bytes read() {
    Busy busy(busy_, sock_, close_pending_);
    Io io = run_unlocked([&]() -> Io {
      while (!eof_ && sock_.is_open()) {
        Io r = fill();
        if (!r) return r;
      }
      return Io{};
    });
    if (!io) {
      sock_.close();
      raise_io(io, &parser_);
    }
    py::bytes rest(buf_.data() + pos_, buf_.size() - pos_);
    consume(buf_.size());
    return rest;
  }

  void close() {
    if (busy_) {
      close_pending_ = true;
      sock_.shutdown();
    } else {
      sock_.close();
    }
  }

  bool closed() const { return !sock_.is_open(); }
  int fileno() const { return sock_.fd(); }

 private:
  // One receive into the parser; de-framed body bytes move to buf_.  The end
  // of the response and the end of the connection both end the stream.
  Io fill() {
    bool eof = false;
    Io r = recv_some(sock_, rbuf_, parser_, &eof);
    if (!r) return r;
    if (eof) {
      parser_.finish_eof();
      eof_ = true;
    }
    if (!parser_.body().empty()) {
      buf_.append(parser_.body());
      parser_.body().clear();
    }
    if (parser_.done()) eof_ = true;
    return Io{};
  }

  // buf_[pos_:] is unread, buf_[scan_:] has not been searched for '\n'
  void consume(size_t end) {
    pos_ = end;
    scan_ = end;
    if (pos_ == buf_.size()) {
      buf_.clear();
      pos_ = scan_ = 0;
    } else if (pos_ > (64u << 10)) {
      buf_.erase(0, pos_);
      pos_ = scan_ = 0;
    }
  }

  Sock sock_;
  ResponseParser parser_;
  std::vector<char> rbuf_;
  std::string buf_;
  size_t pos_ = 0, scan_ = 0;
  bool eof_ = false;
  bool busy_ = false;
  bool close_pending_ = false;
};

// ---- ResponseParser for callers that own the socket (TLS) ------------------
class PyResponseParser {
 public:
  explicit PyResponseParser(bool head_request) : parser_(head_request) {}

  // True once the response is complete; raises what http.client would.
  bool feed(py::buffer b) {
    py::buffer_info info = b.request();
    if (info.ndim > 1) throw py::type_error("expected a flat buffer");
    Feed f = parser_.feed(static_cast<const char *>(info.ptr),
                          static_cast<size_t>(info.size * info.itemsize));
    if (f == Feed::error) raise_parse(parser_);
    return f == Feed::done;
  }
  bool finish_eof() {
    if (parser_.finish_eof() == Feed::error) raise_parse(parser_);
    return true;
  }
  py::tuple result() const {
    if (!parser_.done()) {
      PyErr_SetString(PyExc_RuntimeError, "response not complete");
      throw py::error_already_set();
    }
    return py::make_tuple(
        parser_.status(),
        py::bytes(parser_.body().data(), parser_.body().size()),
        parser_.keep_alive());
  }
  void reset(bool head_request) { parser_.reset(head_request); }

 private:
  ResponseParser parser_;
};

py::bytes py_build_head(py::object method, py::object path, py::object host,
                        py::object headers, py::object body_len) {
  int64_t n = body_len.is_none() ? -1 : body_len.cast<int64_t>();
  if (!body_len.is_none() && n < 0) throw py::value_error("negative body length");
  return py::bytes(make_head(method, path, to_wire(host, true), headers, n));
}

PyObject *lookup(const char *mod, const char *name) {
  py::object o = py::module_::import(mod).attr(name);
  return o.release().ptr();
}

}  // namespace

PYBIND11_MODULE(_httprt, m) {
  m.doc() = "keep-alive HTTP/1.1 round trips with the GIL released";

  g_RemoteDisconnected = lookup("http.client", "RemoteDisconnected");
  g_BadStatusLine = lookup("http.client", "BadStatusLine");
  g_IncompleteRead = lookup("http.client", "IncompleteRead");
  g_LineTooLong = lookup("http.client", "LineTooLong");
  g_HTTPException = lookup("http.client", "HTTPException");
  g_gaierror = lookup("socket", "gaierror");

  py::class_<Conn>(m, "Conn")
      .def(py::init<const std::string &, int, py::object>(), py::arg("host"),
           py::arg("port"), py::arg("timeout_s") = py::none())
      .def("roundtrip", &Conn::roundtrip, py::arg("method"), py::arg("path"),
           py::arg("headers") = py::none(), py::arg("body") = py::none())
      .def("close", &Conn::close)
      .def("fileno", &Conn::fileno)
      .def_property_readonly("closed", &Conn::closed)
      .def_property_readonly("keep_alive", &Conn::keep_alive);

  py::class_<LineStream>(m, "LineStream")
      .def(py::init<const std::string &, int, py::object, py::object,
                    py::object, py::object>(),
           py::arg("host"), py::arg("port"), py::arg("timeout_s"),
           py::arg("path"), py::arg("headers") = py::none(),
           py::arg("method") = py::str("GET"))
      .def_property_readonly("status", &LineStream::status)
      .def("readline", &LineStream::readline)
      .def("read", &LineStream::read)
      .def("close", &LineStream::close)
      .def("fileno", &LineStream::fileno)
      .def_property_readonly("closed", &LineStream::closed);

  py::class_<PyResponseParser>(m, "ResponseParser")
      .def(py::init<bool>(), py::arg("head_request") = false)
      .def("feed", &PyResponseParser::feed)
      .def("finish_eof", &PyResponseParser::finish_eof)
      .def("result", &PyResponseParser::result)
      .def("reset", &PyResponseParser::reset, py::arg("head_request") = false);

  m.def("build_head", &py_build_head, py::arg("method"), py::arg("path"),
        py::arg("host"), py::arg("headers") = py::none(),
        py::arg("body_len") = py::none());
  m.def("host_header", &httpwire::host_header, py::arg("host"),
        py::arg("port"), py::arg("default_port"));
}
