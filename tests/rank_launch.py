"""The launcher of the by-rank GPU tests: one fresh child process per rank on 127.0.0.1 (never an exec of the current process), killed
if it outlives the time limit, every exit status checked.  A plain module imported by name; the ranks share the visible GPU(s)."""

import os
import socket
import subprocess
import sys

import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))


def run_ranks(world, worker, need, timeout, omp_threads=8, **extra_env):
    """tests/<worker> once per rank, with the rendezvous variables, OMP_NUM_THREADS = omp_threads and extra_env in its environment;
    every rank must exit with 0 inside `timeout` seconds and rank 0 must have printed every tag of `need` -> the output of rank 0"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OMP_NUM_THREADS=str(omp_threads), HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
        procs.append(subprocess.Popen([sys.executable, os.path.join(TESTS, worker)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        outs = [p.communicate(timeout=timeout)[0] for p in procs]
    finally:
        for p in procs:  # (exactly the processes started here)
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    assert all(tag in outs[0] for tag in need), outs[0][-3000:]
    return outs[0]
