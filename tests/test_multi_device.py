"""smh_multi_*: one process driving several GPUs -- byte-range shards resident per device, kernels side by side,
ONE RCCL all-reduce of the 64-bit counts (the reference's MPI_Scatterv / MPI_Reduce, main.c:464-489, 654-657).

CPU box: the entry points exist and fail cleanly without a device.  GPU box: with one device the whole path runs
with an RCCL communicator of one rank; with two or more devices visible the shards really spread (skipped at one)."""
import os
import sys

import numpy as np
import pytest

from perf import perf_check

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cuda-aho-corasick-wu-manber_amd"))
import smatcher_hip as S  # noqa: E402


def test_multi_entry_points_exist_and_fail_cleanly_without_devices():
    for name in ("smh_multi_create", "smh_multi_device_count", "smh_multi_uses_rccl", "smh_multi_load_text",
                 "smh_multi_generate_text", "smh_multi_ac_count", "smh_multi_wm_count", "smh_multi_free"):
        getattr(S.lib, name)
    if S.device_count() == 0:
        with pytest.raises(S.SmhError, match="visible"):
            S.MultiGpu(1)
    with pytest.raises(S.SmhError):
        S.MultiGpu(0)
    with pytest.raises(S.SmhError):
        S.MultiGpu(2, devices=[0, 0])  # a device twice / not visible: refused either way (SMH_MULTI_SHARE_DEVICE rehearses it)


def _case(n, m, p, sigma):
    text = S.corpus_text(n, 42, sigma)
    pat = S.corpus_patterns(m, p, 7, sigma, 42, n, 2)
    want, _ = O.oracle_ac(pat, m, p, sigma, text)
    return text, pat, want


@pytest.mark.gpu
@pytest.mark.parametrize("n_devices", [1, 2, 4, 8])
def test_multi_device_counts_match_the_oracle(n_devices):
    """With fewer cards than shards the N-device flow is REHEARSED on what is there (SMH_MULTI_SHARE_DEVICE: logical shard i
    on device i mod the visible ones; per-shard streams, text ranges, counters and -- by the runtime's slot keys -- table
    sets; host-side sum, since an RCCL communicator takes a device once): shard placement with the last shard's true
    length, per-shard counts == the oracle's count of the main.c:467-477 range, the halo refusal."""
    share = S.device_count() < n_devices
    n, m, p, sigma = 6_000_007, 16, 500, 4
    text, pat, want = _case(n, m, p, sigma)
    mg = S.MultiGpu(n_devices, flags=S.MULTI_SHARE_DEVICE if share else 0)
    assert mg.devices == n_devices and mg.uses_rccl == (not share)
    mg.load_text(text, 63)
    ac = S.AcAutomaton.from_patterns(pat, m, p, sigma)
    wm = S.WmTables.from_patterns(pat, m, p, sigma)
    for handle, fn in ((ac, mg.ac_count), (wm, mg.wm_count)):
        total, per, secs = fn(handle)
        assert total == want and sum(per) == want and len(per) == n_devices and secs > 0
        # every device's count is the oracle's count of its byte range (main.c:467-477)
        for r in range(n_devices):
            b, e = S.shard_range(n, n_devices, r, m)
            assert per[r] == O.oracle_ac(pat, m, p, sigma, text[b:e])[0]
    # a second, shorter pattern set over the SAME resident shards; a longer one than the halo is refused
    pat8 = S.corpus_patterns(8, 100, 9, sigma, 42, n, 2)
    ac8 = S.AcAutomaton.from_patterns(pat8, 8, 100, sigma)
    assert mg.ac_count(ac8)[0] == O.oracle_ac(pat8, 8, 100, sigma, text)[0]
    pat65 = S.corpus_patterns(65, 10, 9, sigma, 42, n, 2)
    with pytest.raises(S.SmhError, match="halo"):
        mg.ac_count(S.AcAutomaton.from_patterns(pat65, 65, 10, sigma))
    # the synthetic corpus generated shard by shard on the devices equals the host corpus
    mg.generate_text(n, 42, sigma, 31)
    assert mg.ac_count(ac)[0] == want
    # host-side sum instead of the communicator: same numbers
    mg2 = S.MultiGpu(n_devices, flags=S.MULTI_NO_RCCL | (S.MULTI_SHARE_DEVICE if share else 0))
    assert not mg2.uses_rccl
    mg2.load_text(text, 15)
    assert mg2.ac_count(ac)[0] == want
    mg2.close()
    mg.close()


@pytest.mark.gpu
@pytest.mark.perf
def test_first_count_call_is_as_fast_as_the_tenth_after_prepare():
    """smh_multi_*_prepare (and the count calls themselves, before their clock starts) build the table set and run
    the kernel once per device: `seconds` of the first count call holds launches + reduce only."""
    n, m, p, sigma = 64 << 20, 16, 1000, 4
    pat = S.corpus_patterns(m, p, 7, sigma, 42, n, 2)
    mg = S.MultiGpu(1)
    mg.generate_text(n, 42, sigma, 31)
    for make, count in ((S.AcAutomaton, mg.ac_count), (S.WmTables, mg.wm_count)):
        h = make.from_patterns(pat, m, p, sigma)
        mg.prepare(h)
        runs = [count(h) for _ in range(10)]
        later = sorted(r[2] for r in runs[1:])[len(runs) // 2]
        perf_check(runs[0][2] <= 2.0 * later + 2e-4, "first smh_multi count call after prepare %.6f s, later ones %.6f s" % (runs[0][2], later))
        assert len({r[0] for r in runs}) == 1
        # without the explicit call the count does the same before its clock starts
        h2 = make.from_patterns(pat, m, p, sigma)
        first = count(h2)
        assert first[0] == runs[0][0]
        perf_check(first[2] <= 2.0 * later + 2e-4, "first smh_multi count call without prepare %.6f s, later ones %.6f s" % (first[2], later))
    mg.close()


def _testing_lib():
    """the product library with the runtime's test hooks compiled in (make emu: -DSMH_TESTING) -- libsmatcher_hip.so carries none"""
    path = os.path.join(ROOT, "tests", "emu", "libsmatcher_hip_testing.so")
    T = S.C.CDLL(path)
    T.smh_wm_compile.restype = S.C.c_void_p
    T.smh_wm_compile.argtypes = [S.u8p, S.C.c_int, S.C.c_int, S.C.c_int]
    T.smh_wm_prepare_device.argtypes = [S.C.c_void_p]
    T.smh_wm_free.argtypes = [S.C.c_void_p]
    T.smh_wm_free.restype = None
    T.smh_dev_build_peak.argtypes = [S.C.c_int]
    return T


def test_product_library_has_no_test_hooks():
    with pytest.raises(AttributeError):
        S.lib.smh_dev_build_peak
    T = _testing_lib()
    T.smh_dev_build_peak(1)  # the twin is loaded once per process: GPU tests before this one may have built table sets through it
    assert T.smh_dev_build_peak(0) == 0


def test_product_library_reads_no_development_knob():
    """Round 6: SMH_WM_TUNE / SMH_AC_TUNE / SMH_HASH_TUNE / SMH_KEY_TUNE / SMH_PSET_TUNE -- some of whose words change the COUNT
    ("nohalo=1", "stmin=-1", "drop=1": timing experiments) -- are compiled only into the testing twin (csrc/smh_tune.h).  The product
    binary holds none of the names, no setter, and the only environment variables it knows are the three count-preserving ones
    include/smatcher_hip.h lists."""
    import re
    blob = open(S.LIB_PATH, "rb").read()
    words = set(w.decode() for w in re.findall(rb"[ -~]{4,}", blob))
    bad = [w for w in words if re.search(r"nohalo|stmin=|drop=1|SMH_(WM|AC|HASH|KEY|PSET)_TUNE|SMH_TEST|gram=|grouped=force|flatk=|regv=|lane0=", w)]
    assert bad == []
    env_names = sorted(w for w in words if re.fullmatch(r"SMH_[A-Z0-9_]+", w))
    assert env_names == ["SMH_ADAPT", "SMH_HOST_PIECE_KIB", "SMH_MULTI_SHARE_DEVICE"]
    with pytest.raises(AttributeError):
        S.lib.smh_test_tune_set
    with pytest.raises(S.SmhError):
        S.tune(S.TUNE_WM, "gram=6")
    # ... and the testing twin does have them
    T = S.load_testing()
    tblob = open(T.LIB_PATH, "rb").read()
    assert b"SMH_WM_TUNE" in tblob and b"nohalo=1" in tblob
    T.tune(T.TUNE_WM, "gram=0")
    T.tune_clear()


def test_knob_forces_a_form_in_the_testing_twin_only(knob, monkeypatch):
    """the same patterns compiled by both libraries with SMH_WM_TUNE exported AND the twin's knob set: only the twin obeys"""
    T = knob.T
    knob.wm("gram=2")  # hashed byte grams where the cost model takes the flat form
    pat = S.corpus_patterns(6, 100000, 7, 256, 42, 1 << 20, 2)
    forced = T.WmTables.from_patterns(pat, 6, 100000, 256)
    plain = S.WmTables.from_patterns(pat, 6, 100000, 256)
    assert forced.info().gram_kind == 2 and plain.info().gram_kind == 9  # (the flat set, since round 6 in its 143.9 KiB table)


@pytest.mark.gpu
def test_table_sets_of_two_handles_are_built_side_by_side(monkeypatch):
    """ensure_device_set builds outside the process-wide mutex: two host threads preparing two handles overlap
    (smh_dev_build_peak counts the builds in flight together).  SMH_TEST_BUILD_DELAY_MS stretches every build by 150 ms
    so that the overlap does not depend on scheduling luck: with the mutex held across the build the second thread
    could not even start its own.  Two threads that prepare the SAME handle on the same device build ONE set: the second
    waits for the first (round 4; it used to build a second copy and free the loser's)."""
    import threading
    T = _testing_lib()
    monkeypatch.setenv("SMH_TEST_BUILD_DELAY_MS", "150")
    n, sigma = 1 << 20, 256

    def compile_one(seed):
        pat = np.ascontiguousarray(S.corpus_patterns(12, 20000, seed, sigma, 42, n, 2))
        h = T.smh_wm_compile(pat.ctypes.data_as(S.u8p), 12, 20000, sigma)
        assert h
        return S.C.c_void_p(h)

    def race(handles):
        T.smh_dev_build_peak(1)
        gate = threading.Barrier(2)
        rcs = [None, None]

        def work(i):
            gate.wait()
            rcs[i] = T.smh_wm_prepare_device(handles[i])
        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        [t.start() for t in th]
        [t.join() for t in th]
        assert rcs == [0, 0]
        return T.smh_dev_build_peak(0)

    a, b = compile_one(11), compile_one(12)
    assert race([a, b]) >= 2
    c = compile_one(13)
    assert race([c, c]) == 1
    for h in (a, b, c):
        T.smh_wm_free(h)


@pytest.mark.gpu
def test_multi_device_shards_of_a_hostile_text():
    """Two shards of 1 GiB of the planted text through the native path (rehearsed on one card when there is one): every
    shard's first launch takes its first look and moves to the plain stride-1 parts on its own (the runtime keeps one
    adaptive state per device and slot); totals and per-shard counts equal a forced engine's count of the same byte ranges."""
    n_devices, m, p, sigma = 2, 32, 1000, 4
    n = 2 << 30
    text = S.corpus_text(n, 42, sigma, 0, S.CORPUS_PLANTED)
    pat = S.corpus_patterns(m, p, 7, sigma, 42, n, 2, S.CORPUS_PLANTED)
    share = S.device_count() < n_devices
    mg = S.MultiGpu(n_devices, flags=S.MULTI_SHARE_DEVICE if share else 0)
    mg.load_text(text, m - 1)
    ac = S.AcAutomaton.from_patterns(pat, m, p, sigma)
    total, per, secs = mg.ac_count(ac)
    total2, per2, secs2 = mg.ac_count(ac)
    assert (total2, list(per2)) == (total, list(per)) and secs2 < secs  # the second call runs the engine the first one settled on
    ref = S.AcAutomaton.from_patterns(pat, m, p, sigma)
    ref.set_scan_engine(S.ENGINE_AC_FLAT)
    for r in range(n_devices):
        b, e = S.shard_range(n, n_devices, r, m)
        assert per[r] == ref.count_host(text[b:e])[0]
    assert total == sum(per)
    ref.close()
    ac.close()
    mg.close()
    S.lib.smh_host_path_release()
