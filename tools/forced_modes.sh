# The MSM suites again under the library's forced modes (nothing of this is the default configuration):
#   BLAZE_SORT_HIDE=2 (the three-level sort always) / 0 (never hidden; the tests that assert a hidden sort are left out) and
#   BLAZE_MSM_PIECES=3 (every task in three pieces: device-resident ones too)
sel="not bench and not thread and not monkey and not random_call and not 2e26 and not full_size and not largest and not dense_walk and not distributions and not host_threads and not switches"
echo "== BLAZE_SORT_HIDE=2"; BLAZE_SORT_HIDE=2 timeout 1500 python -m pytest tests/test_gpu_msm.py tests/test_gpu_msm_stream.py tests/test_gpu_msm_shards.py tests/test_gpu_msm_precompute.py -x -q -k "$sel" 2>&1 | tail -3
echo "== BLAZE_SORT_HIDE=0"; BLAZE_SORT_HIDE=0 timeout 1500 python -m pytest tests/test_gpu_msm.py tests/test_gpu_msm_stream.py tests/test_gpu_msm_shards.py tests/test_gpu_msm_precompute.py -x -q -k "$sel and not hidden and not sorts_under" 2>&1 | tail -3
echo "== BLAZE_MSM_PIECES=3"; BLAZE_MSM_PIECES=3 timeout 1200 python -m pytest tests/test_gpu_msm.py tests/test_gpu_msm_stream.py tests/test_gpu_msm_precompute.py -x -q -k "harness or randomised or hbm_modes or arena or two_in_flight or stream or non_canonical or mixed_window or plan" 2>&1 | tail -3
