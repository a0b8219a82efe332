"""CPU: `TorchCpuNoiseFeed` — the chunked host-side stand-in for the Exp(1) draws `torch.multinomial` makes once per decode
step in the reference (models/ssr.py:85). It must (a) produce the same numbers as per-step draws, whatever the chunking,
(b) leave the generator where the reference leaves it after exactly n steps, (c) behave the same for the global generator
and for a private `torch.Generator` seeded alike (the contract of `inference_batch`: row i == a batch-1 run after
`torch.manual_seed(seed + i)`). Below: `noise_segments` and the draw half of `NoiseUploader`, through which both decode loops use it."""
import pytest
import torch

import ssr_speech_amd  # noqa: F401
from ssr_speech_amd.engine import NoiseUploader, TorchCpuNoiseFeed, noise_segments

K, CARD = 4, 2056


def per_step(n, generator=None):
    return torch.stack([torch.empty(K, CARD).exponential_(1, generator=generator) for _ in range(n)]) if n else torch.empty(0, K, CARD)


@pytest.mark.parametrize("chunks", [[16, 16, 16], [1, 5, 64, 3], [37]])
def test_chunked_draws_equal_per_step_draws_global_generator(chunks):
    n = sum(chunks)
    torch.manual_seed(123)
    torch.randint(0, 101, (1, 30))                    # the uncond_x draw that precedes sampling (ssr.py:574)
    want = per_step(n)
    after = torch.get_rng_state()
    torch.manual_seed(123)
    torch.randint(0, 101, (1, 30))
    feed = TorchCpuNoiseFeed([None], K, CARD)
    got = []
    for c in chunks:
        buf = torch.empty(c, K, CARD)
        feed.draw(0, buf)
        got.append(buf)
    assert torch.equal(torch.cat(got), want)
    assert torch.equal(torch.get_rng_state(), after)


@pytest.mark.parametrize("n_taken", [0, 1, 16, 17, 40, 47, 48])
def test_finish_rewinds_to_the_state_after_exactly_n_steps(n_taken):
    torch.manual_seed(7)
    per_step(n_taken)
    want_state = torch.get_rng_state()
    want_next = torch.rand(3)
    torch.manual_seed(7)
    feed = TorchCpuNoiseFeed([None], K, CARD)
    for _ in range(3):                                 # 48 steps drawn ahead, only n_taken consumed
        feed.draw(0, torch.empty(16, K, CARD))
    feed.finish(0, n_taken)
    assert torch.equal(torch.get_rng_state(), want_state)
    assert torch.equal(torch.rand(3), want_next)


def test_private_generators_match_the_global_stream_and_do_not_interact():
    seeds = [1000, 1001]
    want = []
    for s in seeds:
        torch.manual_seed(s)
        u = torch.randint(0, 101, (1, 12))
        want.append((u, per_step(20)))
    gens = [torch.Generator().manual_seed(s) for s in seeds]
    unc = [torch.randint(0, 101, (1, 12), generator=g) for g in gens]
    feed = TorchCpuNoiseFeed(gens, K, CARD)
    got = [[], []]
    for _ in range(2):                                 # interleaved chunks, as the engine draws them
        for u in range(2):
            buf = torch.empty(10, K, CARD)
            feed.draw(u, buf)
            got[u].append(buf)
    for u in range(2):
        assert torch.equal(unc[u], want[u][0])
        assert torch.equal(torch.cat(got[u]), want[u][1])
    feed.finish(0, 13)
    ref = torch.Generator().manual_seed(seeds[0])
    torch.randint(0, 101, (1, 12), generator=ref)
    per_step(13, generator=ref)
    assert torch.equal(gens[0].get_state(), ref.get_state())


def test_self_check_and_the_per_step_fallback(monkeypatch):
    """the chunked draw is an assumption about this torch build — the feed checks it once per shape and, on a build where
    it fails, draws step by step into the same staging buffer (same numbers, same generator end state, `finish` included)."""
    assert TorchCpuNoiseFeed.chunked_draws_match(K, CARD) is True            # this image's build
    monkeypatch.setitem(TorchCpuNoiseFeed._chunk_ok, (K, CARD), False)      # pretend the build fails the check
    torch.manual_seed(11)
    want = per_step(40)
    torch.manual_seed(11)
    feed = TorchCpuNoiseFeed([None], K, CARD)
    assert feed.chunked is False
    got = []
    for c in (16, 16, 16):
        buf = torch.empty(c, K, CARD)
        feed.draw(0, buf)
        got.append(buf)
    assert torch.equal(torch.cat(got)[:40], want)
    feed.finish(0, 40)
    torch.manual_seed(11)
    per_step(40)
    assert torch.equal(torch.get_rng_state(), torch.get_rng_state())
    ref_next = torch.rand(2)
    torch.manual_seed(11)
    feed2 = TorchCpuNoiseFeed([None], K, CARD)
    for c in (16, 16, 16):
        feed2.draw(0, torch.empty(c, K, CARD))
    feed2.finish(0, 40)
    assert torch.equal(torch.rand(2), ref_next)


# ---------------------------------------------------------------- which steps the decode loops draw next: `noise_segments`
@pytest.mark.parametrize("chunk", [1, 4, 16])
def test_noise_segments_equal_the_lock_step_loops_rule(chunk):
    """`iter_chunks` drew steps [total, min(total + chunk, limit)) of every live slot, and nothing once total >= limit; a live slot has
    drawn exactly the steps enqueued so far."""
    for limit in range(41):
        for total in range(0, limit + chunk, chunk):
            for mask in range(8):
                live = [u for u in range(3) if mask >> u & 1]
                drawn = [total if u in live else 5 for u in range(3)]              # what a dead slot has drawn does not matter
                want = [(u, total, min(total + chunk, limit) - total) for u in live] if total < limit else []
                assert noise_segments(drawn, live, chunk, limit) == want, (limit, total, live)


@pytest.mark.parametrize("max_steps", [16, 21, 48])
@pytest.mark.parametrize("chunk", [1, 4, 16])
def test_noise_segments_equal_the_queue_loops_rule(chunk, max_steps):
    """`iter_queue` drew min(chunk, max_steps - drawn[u]) steps from drawn[u] per slot, skipping a slot with nothing left."""
    for d0 in range(max_steps + 1):
        for d1 in range(max_steps + 1):
            drawn = [d0, 7, d1]
            want = []
            for u in (2, 0):
                n = min(chunk, max_steps - drawn[u])
                if n > 0:
                    want.append((u, drawn[u], n))
            assert noise_segments(drawn, [2, 0], chunk, max_steps) == want, (d0, d1)


def test_uploader_draw_half_through_a_reset_and_an_early_finish():
    """`NoiseUploader.fill` (what `send` does before the copy, here on an unpinned buffer): slot 0 on the global generator runs 11 of a
    limit of 21 steps and finishes early; slot 1 finishes its first utterance after 6 steps, is reset to another generator mid-run and
    runs that one for 9. Every segment holds per-step [K, card] draws and every generator ends after exactly n_taken of them."""
    k, card, chunk, limit = 2, 8, 4, 21
    step = lambda n, g: torch.stack([torch.empty(k, card).exponential_(1, generator=g) for _ in range(n)])
    taken = {"global": 11, "a": 6, "b": 9}
    torch.manual_seed(77)
    want = {"global": step(24, None)}
    torch.manual_seed(77)
    step(taken["global"], None)
    want_state = {"global": torch.get_rng_state()}
    for name, seed in (("a", 5), ("b", 6)):
        want[name] = step(24, torch.Generator().manual_seed(seed))
        ref = torch.Generator().manual_seed(seed)
        step(taken[name], ref)
        want_state[name] = ref.get_state()

    gens = {"a": torch.Generator().manual_seed(5), "b": torch.Generator().manual_seed(6)}
    torch.manual_seed(77)
    feed = TorchCpuNoiseFeed([None, gens["a"]], k, card)
    bufs = [torch.full((2, chunk, k, card), -1.0) for _ in range(3)]
    owner = ["global", "a"]

    def fill(buf_i, slots):
        segs = NoiseUploader.fill(feed, bufs[buf_i], slots, chunk, limit)
        for u, off, n in segs:
            assert torch.equal(bufs[buf_i][u, :n], want[owner[u]][off:off + n]), (owner[u], off, n)
        return segs

    assert fill(2, [0, 1]) == [(0, 0, 4), (1, 0, 4)]                   # the admission buffer, then the ring
    assert fill(0, [0, 1]) == [(0, 4, 4), (1, 4, 4)]
    assert fill(1, [0, 1]) == [(0, 8, 4), (1, 8, 4)]                   # drawn ahead of slot 1's stop at 6
    feed.finish(1, taken["a"])
    assert torch.equal(gens["a"].get_state(), want_state["a"])
    feed.reset_slot(1, gens["b"])
    owner[1] = "b"
    assert fill(2, [1]) == [(1, 0, 4)]
    assert fill(0, [0, 1]) == [(0, 12, 4), (1, 4, 4)]
    assert fill(1, [0, 1]) == [(0, 16, 4), (1, 8, 4)]
    assert fill(0, [0, 1]) == [(0, 20, 1), (1, 12, 4)]                 # slot 0 is cut at the limit
    assert fill(1, [0, 1]) == [(1, 16, 4)]                             # ... and left out beyond it
    feed.finish(0, taken["global"])
    feed.finish(1, taken["b"])
    assert torch.equal(torch.get_rng_state(), want_state["global"])
    assert torch.equal(gens["b"].get_state(), want_state["b"])
    assert torch.equal(gens["a"].get_state(), want_state["a"])         # untouched by the slot's second utterance
