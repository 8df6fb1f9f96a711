"""The stream-ordered device forward's surface, without a GPU: the C ABI entry and its option, the engine method, the
model's opt-in attribute and its environment default."""
import os

from medaka_amd import engine, lib, models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_and_its_option_are_declared():
    header = open(os.path.join(ROOT, "include", "medaka_amd.h")).read()
    assert "int mdk_gru_forward_dev_async(mdk_gru *m, const float *x_dev, int B, int T, float *probs_dev, void *stream);" in header
    assert '"async_depth"' in header
    assert lib.ABI["mdk_gru_forward_dev_async"] == lib.ABI["mdk_gru_forward_dev"]
    assert callable(engine.GruEngine.forward_async_ptr)


def test_stream_ordered_is_opt_in(monkeypatch):
    monkeypatch.delenv("MEDAKA_AMD_STREAM_ORDERED", raising=False)
    assert models.GRUModel().stream_ordered is False
    monkeypatch.setenv("MEDAKA_AMD_STREAM_ORDERED", "1")
    assert models.GRUModel().stream_ordered is True
    monkeypatch.setenv("MEDAKA_AMD_STREAM_ORDERED", "0")
    assert models.GRUModel().stream_ordered is False
