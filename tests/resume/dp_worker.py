"""One rank of tests/resume/test_gpu_parallel.py: ``python dp_worker.py RANK WORLD PORT OUTDIR PHASE [PHASE ...]`` joins a gloo
group on GPU 0 and runs ``train_imagenet.run`` once per phase, all ranks of a phase on ONE log directory, OUTDIR/<name>:

    straight:<name>     4 iterations
    stopped:<name>      2 iterations, a checkpoint after the second
    resumed:<name>      continue <name>'s newest checkpoint to iteration 4
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main(rank, world, port, out, phases):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=port, RANK=rank, WORLD_SIZE=world, LOCAL_RANK=rank,
                      LOANS_DIST_BACKEND='gloo')
    os.environ.setdefault('LOANS_SPLITK', '0')              # the order-preserving kernels, as tests/conftest.py pins them
    os.environ.setdefault('LOANS_TUNE_POLICY', 'fixed')
    import train_imagenet as T
    from loans_amd import parallel
    from tests.resume.test_gpu_parallel import RUN
    for phase in phases:
        kind, name = phase.split(':')
        log_dir = os.path.join(out, name)
        more = {'straight': ['--iterations', '4', '-l', log_dir],
                'stopped': ['--iterations', '2', '--checkpoint-interval', '2', '-l', log_dir],
                'resumed': ['--iterations', '4', '--resume', log_dir]}[kind]
        T.run(T.parse_args(RUN + more), log=lambda *a: None)
    parallel.shutdown()


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5:])
