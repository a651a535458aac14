#!/usr/bin/env python3
"""Cost of one control-plane REST hop, by transport.

One ``FastHTTPServer`` in this process answers a PATCH with a ~300 B JSON
body — the shape of the ASSIGNED patch inside Allocate.  Against it, and
over the same kind of keep-alive loopback connection, three clients are
timed:

  stdlib   HttpSession on ``http.client``      (GPUSHARE_HTTP_NATIVE=0)
  native   HttpSession on ``gpushare_amd._httprt``
  floor    a bare ``sendall``/``recv`` of pre-built request bytes: what the
           socket round trip and the server side cost with no client work

The server thread shares this interpreter, so a client that waits with the
GIL released (native) lets it run sooner than one that waits holding it
between bytecodes; that is why native can come out below the Python floor.

Usage:  python benchmarks/http_roundtrip.py [--n 20000] [--repeat 5]
Prints one JSON line: µs per round trip (median of the repeats) per client.
"""

from __future__ import annotations

import argparse
import json
import os
import socket
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpushare_amd.cluster.fasthttp import FastHTTPServer  # noqa: E402
from gpushare_amd.cluster.httpconn import HttpSession  # noqa: E402

PATH = "/api/v1/namespaces/default/pods/bench-pod-0"
PATCH = json.dumps(
    {"metadata": {"annotations": {"scheduler.framework.gpushare.allocation":
                                  "true", "assume-time": "1700000000000"}}}
).encode()
HEADERS = {"Content-Type": "application/strategic-merge-patch+json"}
REPLY = json.dumps({"kind": "Pod", "metadata": {"name": "bench-pod-0",
                                                "annotations": {"k": "v" * 220}}}).encode()


def session(url: str, native: bool) -> HttpSession:
    old = os.environ.get("GPUSHARE_HTTP_NATIVE")
    os.environ["GPUSHARE_HTTP_NATIVE"] = "1" if native else "0"
    try:
        s = HttpSession(url, headers={"Accept": "application/json"})
    finally:
        if old is None:
            del os.environ["GPUSHARE_HTTP_NATIVE"]
        else:
            os.environ["GPUSHARE_HTTP_NATIVE"] = old
    if native and s._rt is None:
        raise RuntimeError("gpushare_amd._httprt is not built")
    return s


def time_session(s: HttpSession, n: int) -> float:
    req = s.request
    t0 = time.perf_counter()
    for _ in range(n):
        status, body = req("PATCH", PATH, body=PATCH, headers=HEADERS)
    dt = time.perf_counter() - t0
    assert status == 200 and body == REPLY
    return dt / n * 1e6


def time_floor(port: int, n: int) -> float:
    raw = (
        f"PATCH {PATH} HTTP/1.1\r\nHost: 127.0.0.1:{port}\r\n"
        f"Accept-Encoding: identity\r\nContent-Length: {len(PATCH)}\r\n"
        "Accept: application/json\r\n"
        "Content-Type: application/strategic-merge-patch+json\r\n\r\n"
    ).encode() + PATCH
    sock = socket.create_connection(("127.0.0.1", port))
    sock.setsockopt(socket.IPPROTO_TCP, socket.TCP_NODELAY, 1)
    sock.sendall(raw)
    want = len(sock.recv(65536))       # whole reply arrives in one segment
    t0 = time.perf_counter()
    for _ in range(n):
        sock.sendall(raw)
        got = 0
        while got < want:
            got += len(sock.recv(65536))
    dt = time.perf_counter() - t0
    sock.close()
    return dt / n * 1e6


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()

    srv = FastHTTPServer(lambda m, p, b: (200, REPLY)).start()
    url = f"http://127.0.0.1:{srv.port}"
    stdlib, native = session(url, False), session(url, True)
    samples: dict[str, list[float]] = {"stdlib": [], "native": [], "floor": []}
    try:
        time_session(stdlib, 500), time_session(native, 500)   # warm up
        for _ in range(args.repeat):                           # interleaved
            samples["stdlib"].append(time_session(stdlib, args.n))
            samples["native"].append(time_session(native, args.n))
            samples["floor"].append(time_floor(srv.port, args.n))
    finally:
        stdlib.close()
        native.close()
        srv.stop()
    out = {
        "bench": "http_roundtrip",
        "unit": "us_per_roundtrip",
        "n": args.n,
        "repeat": args.repeat,
        "request_body_bytes": len(PATCH),
        "response_body_bytes": len(REPLY),
    }
    for k, v in samples.items():
        out[k] = round(statistics.median(v), 2)
        out[k + "_min_max"] = [round(min(v), 2), round(max(v), 2)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
