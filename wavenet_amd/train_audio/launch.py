"""``--gpus N`` (new; the reference is single-device): the command line's way into ``wavenet_amd/dp.py``.

The command the user typed becomes the PARENT: it checks the flag, starts ``torch.distributed.run`` with N ranks of the same
module and the same arguments as a child process, and exits with its code.  The parent makes no HIP call and no ``torch.cuda``
query, and replaces its program with nothing.  Every rank then calls ``join`` before it builds a model.  One node; a rank
that fails takes the others down with it (``torch.distributed.run`` does that, and nothing here retries or restarts).

This module imports torch only inside ``join`` and what follows it: ``command`` and the checks are pure."""
from __future__ import annotations

import contextlib
import datetime
import os
import socket
import subprocess
import sys

MIN_GPUS, MAX_GPUS = 1, 8
SHARE_GPU = "WAVENET_DP_SHARE_GPU"      # test hook: "1" puts every rank on --gpu_device over gloo (the one-GPU rehearsal)
TIMEOUT_S = 1800                        # of every collective: a lost rank ends the run instead of hanging it


def check_gpus(n):
    """1 .. 8, or a ValueError that names the value."""
    if not (MIN_GPUS <= int(n) <= MAX_GPUS):
        raise ValueError("--gpus must lie in %d .. %d (the GPUs of one node), got %d" % (MIN_GPUS, MAX_GPUS, int(n)))
    return int(n)


def check_batch(batch_size, n):
    """``--batch-size`` is the global batch: it must divide by the ranks, or a ValueError that names both."""
    if int(batch_size) % int(n):
        raise ValueError("--batch-size %d does not divide by --gpus %d: the batch size is the global batch, every rank takes "
                         "an equal share of it" % (int(batch_size), int(n)))
    return int(batch_size) // int(n)


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def command(module, argv, n, port):
    """The child's command line: N ranks of ``python -m module argv...`` on this node."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(check_gpus(n)),
            "--master-addr", "127.0.0.1", "--master-port", str(int(port)), "-m", str(module)] + [str(a) for a in argv]


def environment(environ=None):
    """The ranks' environment: the caller's, with what bench.py sets for its ranks."""
    env = dict(os.environ if environ is None else environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")          # dmabuf IPC (RCCL needs it)
    env.setdefault("OMP_NUM_THREADS", "8")
    return env


def in_rank() -> bool:
    """Whether this process was started by a launcher (``torch.distributed.run`` sets WORLD_SIZE)."""
    return "WORLD_SIZE" in os.environ


def run(module, argv, n) -> int:
    """Start the N ranks as a child process, wait, return its exit code."""
    return subprocess.call(command(module, argv, n, free_port()), env=environment())


def join(args):
    """Inside a rank, before a model is built: -> (rank, world).  The rank's device is ``args.gpu_device + LOCAL_RANK`` and
    ``args.gpu_device`` is set to it, so that ``model.build`` puts the network there; the group is RCCL (backend "nccl") with that
    device.  Under the test hook every rank stays on ``args.gpu_device`` and the group is gloo.  A world of one joins nothing."""
    gpus = check_gpus(getattr(args, "gpus", 1))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank, local = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    if world != gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: start the ranks with --nproc-per-node equal to --gpus (or give --gpus "
                         "alone: the command starts them itself)" % (gpus, world))
    if world == 1:
        return 0, 1
    if args.gpu_device < 0:
        raise SystemExit("--gpu_device %d with --gpus %d: the ranks take devices gpu_device, gpu_device + 1, ..." % (args.gpu_device, gpus))
    import torch
    import torch.distributed as dist
    timeout = datetime.timedelta(seconds=TIMEOUT_S)
    if os.environ.get(SHARE_GPU) == "1":
        torch.cuda.set_device(args.gpu_device)
        dist.init_process_group("gloo", timeout=timeout)
    else:
        args.gpu_device += local
        torch.cuda.set_device(args.gpu_device)
        dist.init_process_group("nccl", device_id=torch.device("cuda", args.gpu_device), timeout=timeout)   # RCCL on ROCm
    return rank, world


def barrier(world):
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


def leave(world):
    """A barrier (rank 0 has written its last file when any rank exits), then the group is taken down."""
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


def shared_seed(seed, rank, world):
    """``--seed`` as every rank must see it: the given one, or one that rank 0 draws and broadcasts."""
    if world == 1 or seed is not None:
        return seed
    import torch.distributed as dist
    box = [int.from_bytes(os.urandom(4), "little") if rank == 0 else None]
    dist.broadcast_object_list(box, src=0)
    return int(box[0])


@contextlib.contextmanager
def rank_stdout(rank):
    """Rank 0 alone prints: the context in which the other ranks' standard output goes nowhere (standard error stays)."""
    if rank == 0:
        yield
        return
    with open(os.devnull, "w") as sink, contextlib.redirect_stdout(sink):
        yield


def build_in_turn(build, rank, world):
    """Rank 0 calls ``build()`` first -- it alone writes wavenet.json, speakers.json and local.json --, a barrier follows, then
    the other ranks build and only read."""
    if rank == 0:
        out = build()
        barrier(world)
        return out
    barrier(world)
    return build()

