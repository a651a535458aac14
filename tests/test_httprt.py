"""The native HTTP transport (gpushare_amd._httprt) behind HttpSession.

Scripted raw-socket servers pin down response framing, the stale keep-alive
retry, timeouts, header-injection refusal and the streaming line reader;
``GPUSHARE_HTTP_NATIVE=0`` sessions give the stdlib ``http.client`` side of
the wire-parity checks.  Everything runs on loopback without a GPU.
"""

from __future__ import annotations

import contextlib
import http.client
import json
import os
import socket
import sys
import threading
import time

import pytest

from gpushare_amd import _httprt
from gpushare_amd.cluster.fakeapiserver import FakeApiServer
from gpushare_amd.cluster.fasthttp import FastHTTPServer
from gpushare_amd.cluster.httpconn import HttpSession
from gpushare_amd.cluster.informer import PodInformer
from gpushare_amd.cluster.kubeclient import FakeKubeClient, RestKubeClient

from helpers import make_pod


# --------------------------------------------------------------------------- #
# scripted server
# --------------------------------------------------------------------------- #

def read_request(conn: socket.socket) -> bytes:
    """One request (head + Content-Length body) as raw bytes; b"" when the
    client hung up."""
    data = b""
    while b"\r\n\r\n" not in data:
        part = conn.recv(65536)
        if not part:
            return b""
        data += part
    head, _, rest = data.partition(b"\r\n\r\n")
    clen = 0
    for line in head.split(b"\r\n")[1:]:
        name, _, value = line.partition(b":")
        if name.strip().lower() == b"content-length":
            clen = int(value)
    while len(rest) < clen:
        part = conn.recv(65536)
        if not part:
            return b""
        rest += part
    return head + b"\r\n\r\n" + rest


class ScriptedServer:
    """Loopback server; ``script(conn, index, server)`` runs once per accepted
    connection on its own thread and the connection is closed when it
    returns.  ``requests`` collects what scripts record."""

    def __init__(self, script):
        self.script = script
        self.connections = 0
        self.requests: list[bytes] = []
        self.lock = threading.Lock()
        self._open: list[socket.socket] = []
        self._sock = socket.socket()
        self._sock.setsockopt(socket.SOL_SOCKET, socket.SO_REUSEADDR, 1)
        self._sock.bind(("127.0.0.1", 0))
        self._sock.listen(64)
        self.port = self._sock.getsockname()[1]
        self.url = f"http://127.0.0.1:{self.port}"
        threading.Thread(target=self._accept, daemon=True).start()

    def _accept(self):
        while True:
            try:
                conn, _ = self._sock.accept()
            except OSError:
                return
            conn.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
            with self.lock:
                index = self.connections
                self.connections += 1
                self._open.append(conn)
            threading.Thread(
                target=self._run, args=(conn, index), daemon=True
            ).start()

    def _run(self, conn, index):
        try:
            self.script(conn, index, self)
        except OSError:
            pass
        finally:
            conn.close()

    def record(self, raw: bytes) -> None:
        with self.lock:
            self.requests.append(raw)

    def stop(self):
        self._sock.close()
        with self.lock:
            for c in self._open:
                try:
                    c.shutdown(socket.SHUT_RDWR)
                except OSError:
                    pass


@pytest.fixture
def serve():
    servers = []

    def make(script):
        s = ScriptedServer(script)
        servers.append(s)
        return s

    yield make
    for s in servers:
        s.stop()


def answering(*responses, one_byte_sends=False):
    """Script: answer request k on a connection with responses[k], then hang
    up."""

    def script(conn, index, server):
        for resp in responses:
            raw = read_request(conn)
            if not raw:
                return
            server.record(raw)
            if one_byte_sends:
                for i in range(len(resp)):
                    conn.sendall(resp[i:i + 1])
            else:
                conn.sendall(resp)

    return script


def ok_response(body: bytes, extra: bytes = b"") -> bytes:
    return (
        b"HTTP/1.1 200 OK\r\n" + extra
        + b"Content-Length: %d\r\n\r\n" % len(body) + body
    )


@contextlib.contextmanager
def transport(native: bool):
    """Sessions made inside use the given transport, whatever the
    environment of the test run says."""
    old = os.environ.get("GPUSHARE_HTTP_NATIVE")
    os.environ["GPUSHARE_HTTP_NATIVE"] = "1" if native else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["GPUSHARE_HTTP_NATIVE"]
        else:
            os.environ["GPUSHARE_HTTP_NATIVE"] = old


def native_session(url, **kw) -> HttpSession:
    with transport(True):
        s = HttpSession(url, **kw)
    assert s._rt is _httprt, "native transport not selected"
    return s


def stdlib_session(url, **kw) -> HttpSession:
    with transport(False):
        s = HttpSession(url, **kw)
    assert s._rt is None
    return s


# --------------------------------------------------------------------------- #
# response framing
# --------------------------------------------------------------------------- #

class TestFraming:
    def test_content_length_empty_and_204_on_one_connection(self, serve):
        srv = serve(answering(
            ok_response(b'{"a":1}', b"Content-Type: application/json\r\n"),
            ok_response(b""),
            b"HTTP/1.1 204 No Content\r\n\r\n",
            ok_response(b"after"),
        ))
        s = native_session(srv.url)
        assert s.request("GET", "/1") == (200, b'{"a":1}')
        assert s.request("GET", "/2") == (200, b"")
        assert s.request("DELETE", "/3") == (204, b"")
        assert s.request("GET", "/4") == (200, b"after")
        assert srv.connections == 1
        s.close()

    def test_chunked_one_byte_per_send(self, serve):
        resp = (
            b"HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n"
            b"5\r\nhello\r\n1\r\n \r\nb\r\nchunked wor\r\n2\r\nld\r\n0\r\n\r\n"
        )
        srv = serve(answering(resp, ok_response(b"next"), one_byte_sends=True))
        s = native_session(srv.url)
        assert s.request("GET", "/c") == (200, b"hello chunked world")
        # the terminating chunk was consumed: the connection is reusable
        assert s.request("GET", "/n") == (200, b"next")
        assert srv.connections == 1
        s.close()

    def test_chunk_extension_and_trailer(self, serve):
        resp = (
            b"HTTP/1.1 200 OK\r\ntransfer-ENCODING: Chunked\r\n\r\n"
            b"4;name=value\r\nabcd\r\nA ; ext\r\n0123456789\r\n"
            b"0;last\r\nX-Checksum: 1234\r\n\r\n"
        )
        srv = serve(answering(resp, ok_response(b"next")))
        s = native_session(srv.url)
        assert s.request("GET", "/c") == (200, b"abcd0123456789")
        assert s.request("GET", "/n") == (200, b"next")
        assert srv.connections == 1
        s.close()

    def test_one_mib_body(self, serve):
        body = bytes(range(256)) * 4096
        srv = serve(answering(ok_response(body)))
        s = native_session(srv.url)
        status, got = s.request("GET", "/big")
        assert status == 200 and got == body
        s.close()

    def test_100_continue_then_200(self, serve):
        srv = serve(answering(
            b"HTTP/1.1 100 Continue\r\n\r\n" + ok_response(b"done")
        ))
        s = native_session(srv.url)
        assert s.request("POST", "/p", body=b"x") == (200, b"done")
        s.close()

    def test_connection_close_then_transparent_reconnect(self, serve):
        def script(conn, index, server):
            server.record(read_request(conn))
            conn.sendall(ok_response(b"conn%d" % index, b"Connection: close\r\n"))

        srv = serve(script)
        s = native_session(srv.url)
        assert s.request("GET", "/a") == (200, b"conn0")
        assert s.request("GET", "/b") == (200, b"conn1")
        assert srv.connections == 2
        s.close()

    def test_body_to_eof_is_not_reused(self, serve):
        def script(conn, index, server):
            server.record(read_request(conn))
            conn.sendall(b"HTTP/1.1 200 OK\r\n\r\nuntil eof %d" % index)

        srv = serve(script)
        s = native_session(srv.url)
        assert s.request("GET", "/a") == (200, b"until eof 0")
        assert s.request("GET", "/b") == (200, b"until eof 1")
        assert srv.connections == 2
        s.close()

    def test_malformed_status_line(self, serve):
        srv = serve(answering(b"SSH-2.0-OpenSSH_9.6\r\n"))
        s = native_session(srv.url)
        with pytest.raises(http.client.BadStatusLine):
            s.request("GET", "/")
        s.close()

    def test_connection_refused(self):
        probe = socket.socket()
        probe.bind(("127.0.0.1", 0))
        port = probe.getsockname()[1]
        probe.close()
        s = native_session(f"http://127.0.0.1:{port}")
        with pytest.raises(ConnectionRefusedError):
            s.request("GET", "/")
        s.close()


# --------------------------------------------------------------------------- #
# stale keep-alive retry, timeout, close
# --------------------------------------------------------------------------- #

class TestRetryAndTimeout:
    def test_stale_pooled_connection_is_retried_once(self, serve):
        # every connection answers one request, then the server hangs up
        srv = serve(answering(ok_response(b"ok")))
        s = native_session(srv.url)
        assert s.request("GET", "/1") == (200, b"ok")
        for _ in range(200):   # until the FIN has arrived on loopback
            if srv.connections == 1 and not _peer_open(s):
                break
            time.sleep(0.005)
        assert s.request("POST", "/2", body=b"{}") == (200, b"ok")
        assert srv.connections == 2
        assert [r.split(b" ")[1] for r in srv.requests] == [b"/1", b"/2"]
        s.close()

    def test_close_on_fresh_connection_raises(self, serve):
        def script(conn, index, server):
            server.record(read_request(conn))   # ...and hang up unanswered

        srv = serve(script)
        s = native_session(srv.url)
        with pytest.raises(http.client.RemoteDisconnected):
            s.request("POST", "/once", body=b"{}")
        assert srv.connections == 1 and len(srv.requests) == 1
        s.close()

    def test_timeout_raises_and_does_not_retry(self, serve):
        release = threading.Event()

        def script(conn, index, server):
            server.record(read_request(conn))
            release.wait(10)

        srv = serve(script)
        s = native_session(srv.url, timeout=0.2)
        t0 = time.monotonic()
        with pytest.raises(socket.timeout):
            s.request("POST", "/slow", body=b"{}")
        elapsed = time.monotonic() - t0
        release.set()
        assert 0.15 <= elapsed < 0.2 + 1.0
        assert srv.connections == 1 and len(srv.requests) == 1

        # also on a POOLED connection: a timeout is never retried
        calls = []

        def script2(conn, index, server):
            server.record(read_request(conn))
            conn.sendall(ok_response(b"first"))
            server.record(read_request(conn))
            calls.append(index)
            release2.wait(10)

        release2 = threading.Event()
        srv2 = serve(script2)
        s2 = native_session(srv2.url, timeout=0.2)
        assert s2.request("GET", "/a") == (200, b"first")
        with pytest.raises(TimeoutError):
            s2.request("POST", "/b", body=b"{}")
        release2.set()
        assert srv2.connections == 1 and len(srv2.requests) == 2
        s.close()
        s2.close()

    def test_close_makes_later_calls_raise(self, serve):
        srv = serve(answering(ok_response(b"ok"), ok_response(b"ok")))
        s = native_session(srv.url)
        assert s.request("GET", "/") == (200, b"ok")
        s.close()
        with pytest.raises(RuntimeError, match="session closed"):
            s.request("GET", "/")

    def test_conn_refuses_a_second_thread(self, serve):
        arrived, release = threading.Event(), threading.Event()

        def script(conn, index, server):
            read_request(conn)
            arrived.set()
            release.wait(10)
            conn.sendall(ok_response(b"late"))

        srv = serve(script)
        conn = _httprt.Conn("127.0.0.1", srv.port, 10.0)
        result = []
        t = threading.Thread(
            target=lambda: result.append(conn.roundtrip("GET", "/", {}, None))
        )
        t.start()
        assert arrived.wait(5)
        with pytest.raises(RuntimeError, match="in use"):
            conn.roundtrip("GET", "/other", {}, None)
        release.set()
        t.join(5)
        assert result == [(200, b"late")]
        conn.close()


def _peer_open(session) -> bool:
    """False once the pooled connection's peer has closed (FIN received)."""
    conn = session._local.conn
    probe = socket.socket(fileno=conn.fileno())
    try:
        probe.setblocking(False)
        try:
            return probe.recv(1, socket.MSG_PEEK) != b""
        except BlockingIOError:
            return True
    finally:
        probe.detach()


# --------------------------------------------------------------------------- #
# injection
# --------------------------------------------------------------------------- #

class TestInjection:
    @pytest.mark.parametrize("path,headers", [
        ("/a\r\nX-Injected: 1", None),
        ("/a\nb", None),
        ("/a b", None),
        ("/ok", {"X-A": "v\r\nX-Injected: 1"}),
        ("/ok", {"X-A": "v\nw"}),
        ("/ok", {"X-A\r\nX-B": "v"}),
        ("/ok", {"X-A": "v\x00w"}),
        ("/café", None),
    ])
    def test_refused_before_anything_is_sent(self, serve, path, headers):
        srv = serve(answering(ok_response(b"1"), ok_response(b"2")))
        s = native_session(srv.url)
        assert s.request("GET", "/first") == (200, b"1")
        with pytest.raises(ValueError):
            s.request("GET", path, headers=headers)
        # nothing reached the server, and the connection is still good
        assert s.request("GET", "/second") == (200, b"2")
        assert srv.connections == 1
        assert [r.split(b" ")[1] for r in srv.requests] == [b"/first", b"/second"]
        s.close()

    def test_refused_on_a_fresh_session_opens_nothing_harmful(self, serve):
        srv = serve(answering(ok_response(b"1")))
        s = native_session(srv.url)
        with pytest.raises(ValueError):
            s.request("GET", "/a\r\nHost: evil")
        assert srv.requests == []
        s.close()


# --------------------------------------------------------------------------- #
# parity with http.client
# --------------------------------------------------------------------------- #

class TestParity:
    CASES = [
        ("GET", "/api/v1/pods?fieldSelector=spec.nodeName%3Dn", None, None),
        ("POST", "/api/v1/namespaces/default/pods",
         b'{"kind":"Pod","metadata":{"name":"p"}}',
         {"Content-Type": "application/json"}),
        ("PATCH", "/api/v1/namespaces/default/pods/p",
         b'{"metadata":{"annotations":{"a":"b"}}}',
         {"Content-Type": "application/strategic-merge-patch+json"}),
        ("DELETE", "/api/v1/namespaces/default/pods/p", None, None),
        ("POST", "/gpushare-scheduler/release", None, None),
        ("PUT", "/x", b"", {"Accept": "text/plain", "X-Int": 7}),
    ]

    def test_same_bytes_on_the_wire_same_results(self, serve):
        def script(conn, index, server):
            while True:
                raw = read_request(conn)
                if not raw:
                    return
                server.record(raw)
                n = len(server.requests)
                status = 404 if raw.startswith(b"DELETE") else 200
                body = json.dumps({"n": n % len(self.CASES)}).encode()
                conn.sendall(
                    b"HTTP/1.1 %d X\r\nContent-Type: application/json\r\n"
                    b"Content-Length: %d\r\n\r\n" % (status, len(body)) + body
                )

        srv = serve(script)
        base = {"Accept": "application/json", "Authorization": "Bearer tok"}
        url = srv.url + "/prefix/"
        results = {}
        for kind in ("native", "stdlib"):
            s = (native_session(url, headers=base) if kind == "native"
                 else stdlib_session(url, headers=base))
            results[kind] = [
                s.request(m, p, body=b, headers=h) for m, p, b, h in self.CASES
            ]
            s.close()
        n = len(self.CASES)
        assert len(srv.requests) == 2 * n
        for i, case in enumerate(self.CASES):
            assert srv.requests[i] == srv.requests[n + i], case
        assert results["native"] == results["stdlib"]
        assert srv.connections == 2
        # spot-check the shape both agree on
        assert srv.requests[1].startswith(
            b"POST /prefix/api/v1/namespaces/default/pods HTTP/1.1\r\n"
            b"Host: 127.0.0.1:%d\r\nAccept-Encoding: identity\r\n"
            b"Content-Length: 38\r\n" % srv.port
        )
        assert b"Content-Length" not in srv.requests[0]
        assert b"Content-Length: 0\r\n" in srv.requests[4]

    def test_build_head_matches_tls_host_rules(self):
        assert _httprt.host_header("example.org", 443, 443) == "example.org"
        assert _httprt.host_header("example.org", 6443, 443) == "example.org:6443"
        head = _httprt.build_head("GET", "/", "example.org", {"A": "b"}, None)
        assert head == (
            b"GET / HTTP/1.1\r\nHost: example.org\r\n"
            b"Accept-Encoding: identity\r\nA: b\r\n\r\n"
        )

    def test_response_parser_object(self):
        p = _httprt.ResponseParser()
        wire = b"HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n3\r\nabc\r\n0\r\n\r\n"
        for i in range(len(wire) - 1):
            assert p.feed(wire[i:i + 1]) is False
        assert p.feed(memoryview(wire)[-1:]) is True
        assert p.result() == (200, b"abc", True)
        p.reset()
        with pytest.raises(http.client.BadStatusLine):
            p.feed(b"garbage\r\n")
        p.reset()
        p.feed(b"HTTP/1.1 200 OK\r\nContent-Length: 9\r\n\r\nabc")
        with pytest.raises(http.client.IncompleteRead):
            p.finish_eof()


# --------------------------------------------------------------------------- #
# threads
# --------------------------------------------------------------------------- #

class CountingFastHTTPServer(FastHTTPServer):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.accepted = 0
        self._count_lock = threading.Lock()

    def _serve_conn(self, conn):
        with self._count_lock:
            self.accepted += 1
        super()._serve_conn(conn)


def test_eight_threads_share_one_session():
    srv = CountingFastHTTPServer(lambda m, p, b: (200, p.encode() + b"|" + b)).start()
    s = native_session(f"http://127.0.0.1:{srv.port}")
    errors = []

    def worker(tid):
        try:
            for i in range(200):
                body = b"t%d-%d" % (tid, i)
                status, got = s.request("POST", f"/echo/{tid}/{i}", body=body)
                if status != 200 or got != f"/echo/{tid}/{i}".encode() + b"|" + body:
                    errors.append((tid, i, status, got))
        except Exception as e:  # noqa: BLE001
            errors.append((tid, repr(e)))

    threads = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(30)
        assert not errors, errors[:5]
        assert 1 <= srv.accepted <= 8
    finally:
        s.close()
        srv.stop()


# --------------------------------------------------------------------------- #
# LineStream
# --------------------------------------------------------------------------- #

def chunk(data: bytes) -> bytes:
    return b"%x\r\n" % len(data) + data + b"\r\n"


STREAM_HEAD = (
    b"HTTP/1.1 200 X\r\nContent-Type: application/json\r\n"
    b"Transfer-Encoding: chunked\r\n\r\n"
)


class TestLineStream:
    def test_lines_across_chunks_and_sends(self, serve):
        wire = (
            STREAM_HEAD
            + chunk(b'{"type":"ADD')            # line split across chunks
            + chunk(b'ED"}\n')
            + chunk(b'{"n":1}\n{"n":2}\n{"n":3}\n')   # several lines, one chunk
            + chunk(b"\n")                        # heartbeat
            + chunk(b"tail without newline")
            + b"0\r\n\r\n"
        )

        def script(conn, index, server):
            server.record(read_request(conn))
            for i in range(len(wire)):            # every split point
                conn.sendall(wire[i:i + 1])

        srv = serve(script)
        s = native_session(srv.url, headers={"Accept": "application/json"})
        conn, resp = s.stream("GET", "/api/v1/pods?watch=true", timeout=5.0)
        assert type(resp).__name__ == "LineStream"
        assert resp.status == 200
        assert resp.readline() == b'{"type":"ADDED"}\n'
        assert resp.readline() == b'{"n":1}\n'
        assert resp.readline() == b'{"n":2}\n'
        assert resp.readline() == b'{"n":3}\n'
        assert resp.readline() == b"\n"
        assert resp.readline() == b"tail without newline"
        assert resp.readline() == b""
        assert resp.readline() == b""
        conn.close()
        assert srv.requests[0].startswith(
            b"GET /api/v1/pods?watch=true HTTP/1.1\r\nHost: 127.0.0.1:%d\r\n"
            b"Accept-Encoding: identity\r\nAccept: application/json\r\n\r\n"
            % srv.port
        )

    def test_eof_when_server_hangs_up_mid_stream(self, serve):
        def script(conn, index, server):
            read_request(conn)
            conn.sendall(STREAM_HEAD + chunk(b"one\n") + b"5\r\ntw")

        srv = serve(script)
        s = native_session(srv.url)
        conn, resp = s.stream("GET", "/w", timeout=5.0)
        assert resp.readline() == b"one\n"
        assert resp.readline() == b"tw"
        assert resp.readline() == b""
        conn.close()

    def test_error_status_body_via_read(self, serve):
        body = b'{"message":"forbidden"}'
        srv = serve(answering(
            b"HTTP/1.1 403 Forbidden\r\nContent-Length: %d\r\n\r\n" % len(body)
            + body
        ))
        s = native_session(srv.url)
        conn, resp = s.stream("GET", "/w", timeout=5.0)
        assert resp.status == 403
        assert resp.read() == body
        assert resp.read() == b""
        conn.close()

    def test_same_lines_as_stdlib_stream(self, serve):
        wire = STREAM_HEAD + chunk(b"a\nbb\n") + chunk(b"c") + chunk(b"cc\n") + b"0\r\n\r\n"

        def script(conn, index, server):
            server.record(read_request(conn))
            conn.sendall(wire)

        srv = serve(script)
        lines = {}
        for kind in ("native", "stdlib"):
            s = (native_session(srv.url) if kind == "native"
                 else stdlib_session(srv.url))
            conn, resp = s.stream("GET", "/w", timeout=5.0)
            got = []
            while True:
                line = resp.readline()
                got.append(line)
                if not line:
                    break
            conn.close()
            lines[kind] = got
        assert lines["native"] == lines["stdlib"] == [b"a\n", b"bb\n", b"ccc\n", b""]
        assert srv.requests[0] == srv.requests[1]

    def test_stream_timeout(self, serve):
        release = threading.Event()

        def script(conn, index, server):
            read_request(conn)
            conn.sendall(STREAM_HEAD + chunk(b"one\n"))
            release.wait(10)

        srv = serve(script)
        s = native_session(srv.url)
        conn, resp = s.stream("GET", "/w", timeout=0.2)
        assert resp.readline() == b"one\n"
        with pytest.raises(socket.timeout):
            resp.readline()
        release.set()
        conn.close()

    def test_informer_over_fake_apiserver(self):
        node = "node-a"
        server = FakeApiServer(store=FakeKubeClient(node_name=node)).start()
        with transport(True):
            kube = RestKubeClient(base_url=server.url)
        assert kube._client._rt is _httprt
        seen = []
        inf = PodInformer(kube, node, on_event=lambda t, o: seen.append(t))
        inf.start()
        try:
            assert inf.wait_synced(5)
            # the fake server subscribes its watch after it has sent the
            # response head: an event published before that is not an event
            # of this stream
            deadline = time.monotonic() + 5
            while time.monotonic() < deadline and not server.store._watchers:
                time.sleep(0.002)
            assert server.store._watchers
            server.store.add_pod(make_pod("p1", node=node, mem=8))
            server.store.patch_pod(
                "default", "p1", {"metadata": {"annotations": {"x": "y"}}}
            )
            server.store.delete_pod("default", "p1")
            deadline = time.monotonic() + 5
            while time.monotonic() < deadline and seen[-1:] != ["DELETED"]:
                time.sleep(0.005)
            assert seen == ["ADDED", "MODIFIED", "DELETED"]
            assert inf.pods() == []
        finally:
            inf.stop()
            server.stop()


# --------------------------------------------------------------------------- #
# fallback
# --------------------------------------------------------------------------- #

class TestFallback:
    def test_session_works_without_the_extension(self, serve, monkeypatch):
        monkeypatch.setitem(sys.modules, "gpushare_amd._httprt", None)
        srv = serve(answering(ok_response(b"one"), ok_response(b"two")))
        with transport(True):
            s = HttpSession(srv.url)
        assert s._rt is None
        assert s.request("GET", "/1") == (200, b"one")
        assert s.request("POST", "/2", body=b"{}") == (200, b"two")
        assert srv.connections == 1
        assert isinstance(s._local.conn, http.client.HTTPConnection)
        s.close()

    def test_env_switch_is_read_per_session(self, serve):
        srv = serve(answering(ok_response(b"x")))
        a = stdlib_session(srv.url)
        b = native_session(srv.url)
        assert a._rt is None and b._rt is _httprt
        assert b.request("GET", "/") == (200, b"x")
        a.close()
        b.close()
