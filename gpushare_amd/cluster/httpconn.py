"""Persistent keep-alive HTTP session; native round trips where built.

The control-plane hot path (Allocate → pending-pod LIST + ASSIGNED PATCH,
extender filter/bind) is 4–6 small localhost/apiserver REST round-trips per
pod.  A general-purpose HTTP stack spends ~0.5–1 ms per request in request
building, header normalization and response model construction — several
times the cost of the actual socket round-trip for sub-KiB bodies.  This
session keeps ONE pooled connection per (session, thread), writes the
request bytes directly, and returns ``(status, body_bytes)`` with zero
response-object overhead.  That transport cost is the floor under the
reference's Allocate p50 too (client-go against the same apiserver,
SURVEY §3.2), so cutting it is a genuine like-for-like win, not a
benchmark trick.

Thread safety: connections are not thread-safe; each thread gets its own
connection via ``threading.local``.  Stale keep-alive sockets (peer
restarted, idle timeout) are retried once on a fresh connection.

Transport: with the ``gpushare_amd._httprt`` extension importable, request
assembly, the socket exchange and response parsing run in C++ with the GIL
released (``native/http_rt.cpp``); for ``https://`` the socket stays an
``ssl.SSLSocket`` and only assembly and parsing are native.  Without the
extension, or with ``GPUSHARE_HTTP_NATIVE=0`` in the environment when the
session is made, everything goes through stdlib ``http.client`` as before.
Both transports put the same bytes on the wire and raise the same
exceptions.
"""

from __future__ import annotations

import http.client
import importlib
import os
import socket
import ssl
import threading
from http.server import ThreadingHTTPServer
from typing import Optional
from urllib.parse import urlparse


class TrackedThreadingHTTPServer(ThreadingHTTPServer):
    """ThreadingHTTPServer whose ``stop_all_connections`` really severs
    every established keep-alive connection.

    ``server_close()`` only closes the *listening* socket; per-connection
    handler threads keep serving already-open keep-alive connections —  a
    'stopped' server that still answers pooled clients.  A real kubelet or
    apiserver restart kills its sockets, so the in-process servers used by
    tests and the bench harness must behave the same for restart/failover
    paths to be testable."""

    daemon_threads = True

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._conn_lock = threading.Lock()
        self._conns: set = set()

    def get_request(self):
        sock, addr = super().get_request()
        with self._conn_lock:
            self._conns = {s for s in self._conns if s.fileno() != -1}
            self._conns.add(sock)
        return sock, addr

    def stop_all_connections(self) -> None:
        with self._conn_lock:
            for s in self._conns:
                try:
                    s.shutdown(socket.SHUT_RDWR)
                except OSError:
                    pass
            self._conns.clear()


def make_ssl_context(verify) -> Optional[ssl.SSLContext]:
    """httpx-style verify: SSLContext → as-is, str → CA file, ``False``
    (explicit!) → no verification, ``None``/``True`` → verified against
    the system store.  Verification is the DEFAULT: only the
    kubelet client opts out explicitly — its serving cert is rarely
    CA-signed and the reference forces insecure there too
    (client.go:75-99) — while apiserver sessions, including long-lived
    watch streams, must not silently run unverified."""
    if isinstance(verify, ssl.SSLContext):
        return verify
    if isinstance(verify, str):
        return ssl.create_default_context(cafile=verify)
    if verify is False:
        ctx = ssl.create_default_context()
        ctx.check_hostname = False
        ctx.verify_mode = ssl.CERT_NONE
        return ctx
    return ssl.create_default_context()


def _load_native():
    """The ``_httprt`` extension module, or None where it is not built."""
    try:
        return importlib.import_module("gpushare_amd._httprt")
    except ImportError:
        return None


class _TlsConn:
    """One TLS connection with ``_httprt.Conn``'s interface: the handshake
    and the record layer stay in ``ssl`` (so verification and ``SSLError``
    behave as with ``HTTPSConnection``), head assembly and response parsing
    are the native ones."""

    def __init__(self, rt, host, port, timeout, ctx):
        self._rt = rt
        self._host_hdr = rt.host_header(host, port, 443)
        self.keep_alive = False
        sock = socket.create_connection((host, port), timeout)
        try:
            sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            self._sock = ctx.wrap_socket(sock, server_hostname=host)
        except BaseException:
            sock.close()
            raise
        self._parser = rt.ResponseParser()
        self._buf = bytearray(65536)

    def roundtrip(self, method, path, headers, body):
        head = self._rt.build_head(
            method, path, self._host_hdr, headers,
            None if body is None else len(body),
        )
        parser, sock, buf = self._parser, self._sock, self._buf
        parser.reset(method.upper() == "HEAD")
        self.keep_alive = False
        sock.sendall(head + body if body else head)
        view = memoryview(buf)
        got = False
        while True:
            n = sock.recv_into(buf)
            if n == 0:
                if not got:
                    raise http.client.RemoteDisconnected(
                        "Remote end closed connection without response"
                    )
                parser.finish_eof()
                break
            got = True
            if parser.feed(view[:n]):
                break
        status, data, self.keep_alive = parser.result()
        return status, data

    def close(self):
        try:
            self._sock.close()
        except OSError:
            pass


class HttpSession:
    """Keep-alive HTTP/1.1 client bound to one base URL."""

    def __init__(
        self,
        base_url: str,
        headers: Optional[dict] = None,
        verify=None,
        timeout: float = 10.0,
    ):
        u = urlparse(base_url)
        if u.scheme not in ("http", "https"):
            raise ValueError(f"unsupported scheme in {base_url!r}")
        self._https = u.scheme == "https"
        self._host = u.hostname or "127.0.0.1"
        self._port = u.port or (443 if self._https else 80)
        self._prefix = u.path.rstrip("/")
        self._timeout = timeout
        self._ctx = make_ssl_context(verify) if self._https else None
        self._headers = dict(headers or {})
        self._local = threading.local()
        self._closed = False
        # read here, not at import: one process can hold sessions of both
        # kinds (parity tests, before/after measurements)
        self._rt = (
            None
            if os.environ.get("GPUSHARE_HTTP_NATIVE", "1") == "0"
            else _load_native()
        )

    # ------------------------------------------------------------------ #
    def _connect(self) -> http.client.HTTPConnection:
        if self._https:
            conn = http.client.HTTPSConnection(
                self._host, self._port, timeout=self._timeout, context=self._ctx
            )
        else:
            conn = http.client.HTTPConnection(
                self._host, self._port, timeout=self._timeout
            )
        self._local.conn = conn
        return conn

    def _connect_native(self):
        if self._https:
            conn = _TlsConn(
                self._rt, self._host, self._port, self._timeout, self._ctx
            )
        else:
            conn = self._rt.Conn(self._host, self._port, self._timeout)
        self._local.conn = conn
        return conn

    def _request_native(self, method, full, body, hdrs) -> tuple[int, bytes]:
        local = self._local
        conn = getattr(local, "conn", None)
        fresh = conn is None
        if fresh:
            conn = self._connect_native()
        for attempt in (0, 1):
            try:
                result = conn.roundtrip(method, full, hdrs, body)
                if not conn.keep_alive:
                    # the server will close (or has closed) its end: the
                    # next request starts on a new connection
                    conn.close()
                    local.conn = None
                return result
            except ValueError:
                # refused before a byte was written (CR/LF in a header,
                # non-ASCII path): the connection is untouched
                raise
            except (
                http.client.RemoteDisconnected,
                http.client.BadStatusLine,
                BrokenPipeError,
                ConnectionResetError,
                ConnectionRefusedError,
                ssl.SSLEOFError,
            ):
                conn.close()
                local.conn = None
                if fresh or attempt == 1:
                    raise
                conn = self._connect_native()
                fresh = True
            except BaseException:
                # a timeout above all: the request reached a live-but-slow
                # server, retrying could double-apply a non-idempotent verb.
                # Whatever it was, this connection's framing is lost.
                conn.close()
                local.conn = None
                raise

    def request(
        self,
        method: str,
        path: str,
        body: Optional[bytes] = None,
        headers: Optional[dict] = None,
    ) -> tuple[int, bytes]:
        """One round-trip; returns (status_code, response_body).

        Retries exactly once on a stale pooled connection — a request that
        died mid-flight on a FRESH connection is raised, not retried (these
        verbs are not all idempotent)."""
        if self._closed:
            raise RuntimeError("session closed")
        hdrs = self._headers if headers is None else {**self._headers, **headers}
        full = self._prefix + path
        if self._rt is not None:
            return self._request_native(method, full, body, hdrs)
        conn = getattr(self._local, "conn", None)
        fresh = conn is None
        if fresh:
            conn = self._connect()
        for attempt in (0, 1):
            try:
                conn.request(method, full, body=body, headers=hdrs)
                resp = conn.getresponse()
                data = resp.read()  # must drain before conn reuse
                return resp.status, data
            except socket.timeout:
                # the request reached a live-but-slow server: retrying
                # could double-apply a non-idempotent verb — surface it
                conn.close()
                self._local.conn = None
                raise
            except (
                http.client.RemoteDisconnected,
                http.client.BadStatusLine,
                http.client.CannotSendRequest,
                BrokenPipeError,
                ConnectionResetError,
                ConnectionRefusedError,
                ssl.SSLEOFError,
            ):
                conn.close()
                self._local.conn = None
                if fresh or attempt == 1:
                    raise
                conn = self._connect()
                fresh = True

    def stream(
        self,
        method: str,
        path: str,
        headers: Optional[dict] = None,
        timeout: Optional[float] = None,
    ) -> tuple[http.client.HTTPConnection, http.client.HTTPResponse]:
        """Open a long-lived streaming request (k8s watch) on a DEDICATED
        connection — never the pooled one, which must stay request/response.
        Caller reads the response incrementally and closes the returned
        connection.

        Over plain http with the native transport both returned objects are
        one ``_httprt.LineStream`` (``status``, ``readline()``, ``read()``,
        ``close()``), whose reader waits with the GIL released."""
        hdrs = self._headers if headers is None else {**self._headers, **headers}
        if self._rt is not None and not self._https:
            ls = self._rt.LineStream(
                self._host, self._port, timeout, self._prefix + path, hdrs,
                method,
            )
            return ls, ls
        if self._https:
            conn = http.client.HTTPSConnection(
                self._host, self._port, timeout=timeout, context=self._ctx
            )
        else:
            conn = http.client.HTTPConnection(
                self._host, self._port, timeout=timeout
            )
        try:
            conn.request(method, self._prefix + path, headers=hdrs)
            resp = conn.getresponse()
        except BaseException:
            conn.close()
            raise
        return conn, resp

    def close(self) -> None:
        self._closed = True
        conn = getattr(self._local, "conn", None)
        if conn is not None:
            conn.close()
            self._local.conn = None
