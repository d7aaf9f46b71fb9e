"""bench.py --full: a plain run measures its headline figure only; the nested runs and the CPU baseline are taken with --full, where each
still applies to the workloads it did and still yields to its --no-* flag (CPU: which measurements a command line selects)."""
import bench


def _extra(*argv, world=1):
    return bench.extra_measurements(bench.parse_args(list(argv)), world)


ALL = {'bf16_saved_tensor', 'masked', 'small', 'fp8_large', 'cpu_baseline'}


def test_plain_run_measures_the_headline_only():
    assert bench.parse_args([]).full is False
    assert _extra() == set()
    assert _extra('--gpus', '1', '--steps', '20', '--warmup', '5') == set()
    assert _extra('--dump-outputs', 'd') == set()
    assert _extra('--config', 'small') == set()
    assert _extra('--gpus', '2', world=2) == set()


def test_full_run_takes_every_nested_measurement_of_the_default_workload():
    assert _extra('--full') == ALL
    assert _extra('--full', '--steps', '3', '--warmup', '1', '--dump-outputs', 'd') == ALL


def test_full_run_yields_to_the_no_flags():
    assert _extra('--full', '--no-cpu-baseline') == ALL - {'cpu_baseline'}
    assert _extra('--full', '--no-masked', '--no-small') == ALL - {'masked', 'small'}
    assert _extra('--full', '--no-bf16-saved', '--no-fp8-large') == ALL - {'bf16_saved_tensor', 'fp8_large'}
    assert _extra('--full', '--bf16-aux') == ALL - {'bf16_saved_tensor'}
    assert _extra('--full', '--no-cpu-baseline', '--no-masked', '--no-bf16-saved', '--no-small', '--no-fp8-large') == set()


def test_full_run_nests_only_where_it_did():
    assert _extra('--full', '--objective', 'masked') == {'cpu_baseline'}
    assert _extra('--full', '--config', 'small') == {'cpu_baseline'}
    assert _extra('--full', '--dtype', 'fp8') == {'masked', 'cpu_baseline'}
    assert _extra('--full', '--dtype', 'f32') == {'masked', 'cpu_baseline'}
    assert _extra('--full', '--gpus', '2', world=2) == set()
