"""Checkpoint/resume semantics: the dispatcher's durable
state is blocked_items.json + appconf.yaml.  Restarting the dispatcher
while the worker keeps running must (a) reload the blocklist from disk,
(b) re-discover the worker and its RESIDENT model via the probe (the
"model survived the proxy restart" path the reference gets from long
keep_alive), and keep serving."""
import json
import os
import socket
import subprocess
import sys
import time

import httpx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "ollamamq_amd", "csrc", "dispatcher",
                   "ollamamq-server")


def _wait_socket(path, timeout=60):
    t0 = time.time()
    while time.time() - t0 < timeout:
        if os.path.exists(path):
            try:
                s = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
                s.connect(path)
                s.close()
                return True
            except OSError:
                pass
        time.sleep(0.2)
    return False


def _start_server(tmp, sock):
    p = subprocess.Popen(
        [BIN, "--no-tui", "-p", "0", "-w", sock, "--probe-interval-ms",
         "300", "-c", os.path.join(tmp, "absent.yaml")],
        stderr=subprocess.PIPE, cwd=tmp, text=True)
    port = int(p.stderr.readline().rsplit(":", 1)[1].split()[0])
    return p, f"http://127.0.0.1:{port}"


def _wait_loaded(base, model, timeout=30):
    deadline = time.time() + timeout
    while time.time() < deadline:
        try:
            b = httpx.get(base + "/admin/models", timeout=2).json()
            if b and b[0]["online"] and model in b[0]["loaded_models"]:
                return True
        except httpx.HTTPError:
            pass
        time.sleep(0.2)
    return False


def test_dispatcher_restart_resumes(tmp_path, sock_dir):
    tmp = str(tmp_path)
    sock = os.path.join(sock_dir, "w.sock")
    worker = subprocess.Popen(
        [sys.executable, "-m", "ollamamq_amd.engine.worker",
         "--socket", sock, "--model", "tiny-cpu", "--max-ctx", "256",
         "--max-batch", "4"],
        cwd=REPO, stdout=subprocess.DEVNULL, stderr=subprocess.STDOUT)
    server = None
    try:
        assert _wait_socket(sock)
        server, base = _start_server(tmp, sock)
        assert _wait_loaded(base, "tiny-cpu")

        # serve one request, then block a user (persists to disk)
        r = httpx.post(base + "/api/generate",
                       json={"model": "tiny-cpu", "prompt": "a",
                             "stream": False,
                             "options": {"num_predict": 2}},
                       timeout=60)
        assert r.status_code == 200
        # block via the same file the TUI writes (x key): simulate by
        # writing the reference-format file, as an operator would migrate
        server.terminate()
        server.wait(timeout=10)
        with open(os.path.join(tmp, "blocked_items.json"), "w") as f:
            json.dump({"users": ["evil"], "ips": []}, f)

        # restart the DISPATCHER only: worker (and its resident model,
        # the in-process analog of long keep_alive) stays up
        server, base = _start_server(tmp, sock)
        assert _wait_loaded(base, "tiny-cpu"), \
            "resident model not re-discovered after dispatcher restart"
        r = httpx.post(base + "/api/chat", json={"model": "tiny-cpu"},
                       headers={"X-User-ID": "evil"}, timeout=10)
        assert r.status_code == 403          # blocklist reloaded
        r = httpx.post(base + "/api/generate",
                       json={"model": "tiny-cpu", "prompt": "b",
                             "stream": False,
                             "options": {"num_predict": 2}},
                       timeout=60)
        assert r.status_code == 200          # serving resumed
    finally:
        if server is not None:
            server.terminate()
        worker.terminate()
