"""The walks of output_walk.py, checked without a GPU: they hold every situation in which the output stage reuses something it kept (the
coverage conditions), and they are sensitive: a fake engine built here, whose caches carry the fields of the real engine's keys
(EdKey, CpKey, DsKey, PsKey, the pitch's resample table per ratio, the two windows' (rate, milliseconds), the span uploads' (rows, W);
supertonic_amd/csrc/engine.hpp, engine_pitch.cpp), delivers
something else than a fresh fake on at least one walk as soon as one field is left out of one key.  The real engine is never edited to
show that.

Three kinds of field cannot be caught by any history, of these walks or others, because no two fetches of one handle differ in them
alone; for those the test asserts exactly that (whenever the shortened key matched, the whole key matched), so that the omission is
shown to be harmless instead of being passed over:
  * hz and Wo of the three keys: a batch's Wo is a function of its width and the rate, and another batch has another seq;
  * buf of the three keys: a grow-only buffer moves only when (rows, Wo) or the pause limit changed, which the key holds already;
  * (rows, W) of the loudness, compressor and de-esser span uploads: the uploaded spans themselves are compared beside the pointer, and
    batches of unlike rows or W have unlike spans.  (The filter's upload holds no spans: there both are caught.)
  * W, B and buf of the shifted rows' key: another batch has another seq, and the pitch scratch moves only when the shape or the ratio
    changed, which seq and gen hold already.

Dither keeps nothing: the fake has no cache for it, and the setting enters only what a PCM16 / PCM24 output truly is (mode, seed, and
whether the stream is a row's or a programme's)."""
import hashlib
import math

import pytest

import output_walk as ow
import pitch_ref

SEED = 0


@pytest.fixture(scope="module")
def walks():
    return ow.walks(SEED)


def _changes(walk, name):
    return [s for s in walk if s[0] == "set" and s[1] == name]


# ---- the generator itself ---------------------------------------------------------------------------------------------------------------------
def test_walks_are_fixed_and_every_step_is_valid(walks):
    assert walks == ow.walks(SEED) and walks != ow.walks(SEED + 1)
    assert 3 <= len(walks) <= 7 and all(10 <= len(w) <= 16 for w in walks), [len(w) for w in walks]
    for w in walks:
        s = ow.start()
        for step in w:
            if step[0] == "set":
                assert step[2] == ow.OFF[step[1]] or step[2] in ow.VALUES[step[1]], step
            elif step[0] == "refuse":
                assert step[2] == ow.refused(s, step[1]) and step[2] not in ow.VALUES.get(step[1], ()), step
            elif step[0] == "op":
                assert step[1] in ow.OPS and step[2] in (0, 1)
            elif step[0] == "fetch":
                assert step[1] in ow.PATHS
            elif step[0] == "batch":
                assert 0 <= step[1] < len(ow.BATCHES)
            t = ow.apply(s, step)
            assert (t == s) == (step[0] in ("op", "refuse", "fetch") or step[2:] == (s.get(step[1]),)), step
            s = t
    # a chain or de-esser drawn is valid at every rate drawn (include/stn.h): no rate change of a walk is refused
    lo, hi = min(ow.VALUES["rate"]), max(ow.VALUES["rate"] + (ow.NATIVE_HZ,))
    for chain in ow.VALUES["filters"]:
        for kind, f, q, g in chain:
            assert f <= 0.45 * lo and f >= hi / (2400.0 if kind in ("highpass", "lowpass") and 0.5 <= q <= 1.5 else 800.0), (kind, f)
    assert all(2000.0 <= d[0] <= 0.45 * lo and d[0] >= hi / 2400.0 for d in ow.VALUES["deesser"])
    assert 1000.0 * ow.PAUSE_S > max(ow.VALUES["pause"]) + 2 * max(t[1] for t in ow.VALUES["trim"])


def test_the_first_five_walks_are_step_for_step_those_from_before_pitch_and_dither(walks):
    """(the ten op families of then are shuffled and dealt as then; what walks 5 and 6 add takes nothing from the others' coverage)"""
    assert all(len(w) == 16 for w in walks[:5])
    assert hashlib.sha1(repr(ow.walks(0)[:5]).encode()).hexdigest() == "25c2934373e33ccc757aca21720d9115228b5fad"
    assert {s[1] for w in walks[:5] for s in w if s[0] == "op"} == set(ow.OPS[:ow.N_SHUFFLED_OPS])
    assert {s[1] for w in walks[5:] for s in w if s[0] == "op"} == set(ow.OPS[ow.N_SHUFFLED_OPS:])


def test_the_pitch_values_are_realised_with_the_ratios_the_fake_keys_its_table_by():
    for v, ab in zip(ow.VALUES["pitch"], ow.PITCH_RATIOS):
        assert abs(v) < 12.0 and pitch_ref.ratio_brute(v) == ab == ow.pitch_ratio(v), (v, ab)
    (a0, b0), (a1, b1), (a2, b2) = ow.PITCH_RATIOS
    assert b0 == b1 and a0 != a1 and a0 == a2 and b0 != b2 and ow.pitch_ratio(None) == (1, 1)
    assert ow.VALUES["dither"][0][0] == ow.VALUES["dither"][1][0] and ow.VALUES["dither"][0][1] != ow.VALUES["dither"][1][1]
    assert {m for m, _ in ow.VALUES["dither"]} == {"round", "tpdf", "tpdf-hp"}


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------------
def test_every_setting_changes_twice_and_goes_on_off_on(walks):
    for name in ow.SETTINGS:
        assert sum(len(_changes(w, name)) for w in walks) >= 2, name
        found = False
        for w in walks:
            on = [s[2] != ow.OFF[name] for s in _changes(w, name)]
            found |= any(on[i] and not on[j] and on[k] for i in range(len(on)) for j in range(i + 1, len(on)) for k in range(j + 1, len(on)))
        assert found, name


def test_every_cached_reuse_situation_occurs(walks):
    flat = [s for w in walks for s in w]
    # two fetches with nothing between them, and again with an op call of each family between them: every step is followed by a full
    # comparison, so a step that changes nothing stands between two fetches of one state
    assert any(s[0] == "fetch" for s in flat) and {s[1] for s in flat if s[0] == "fetch"} <= set(ow.PATHS)
    assert {s[1] for s in flat if s[0] == "op"} == set(ow.OPS) and {s[2] for s in flat if s[0] == "op"} == {0, 1}
    assert len({s[1] for s in flat if s[0] == "refuse"}) >= 2 and ("refuse", "limiter", 11.0) in flat
    assert any(s[0] == "refuse" and s[1] == "filters" and s[2][0][1] > 0.5 * min(ow.VALUES["rate"]) for s in flat)
    # the batch grows (more rows and wider ones: every scratch moves) and shrinks (reused dirty)
    size = lambda i: (len(ow.BATCHES[i][0]), max(ow.BATCHES[i][1]))  # noqa: E731
    grows = shrinks = rows_only = False
    for w in walks:
        at = 0
        for s in w:
            if s[0] == "batch":
                (b0, d0), (b1, d1) = size(at), size(s[1])
                grows |= b1 > b0 and d1 > d0
                shrinks |= b1 < b0 and d1 < d0
                rows_only |= b1 != b0 and d1 == d0
                at = s[1]
    assert grows and shrinks and rows_only
    assert any(s[0] == "wav" for s in flat)
    # a joined fetch of each gain scope directly before a per-row fetch and directly after one, in both orders of the comparison
    for i in (0, 1):
        order = ow.take_order(i)
        assert sorted(order) == sorted(ow.REPORTS + ow.FETCHES)
        for j in ow.JOINED:
            k = order.index(j)
            assert order[k - 1] in ow.PER_ROW and order[k + 1] in ow.PER_ROW, (i, j)
    assert (ow.take_order(0)[0] in ow.REPORTS) and (ow.take_order(1)[0] in ow.FETCHES)
    assert {e for i in range(5) for e in ow.encodings(i)} == set(ow.ENCODINGS) and all(len(set(ow.encodings(i))) == 2 for i in range(5))


def test_rate_changes_alone_and_states_come_back(walks):
    assert any(len(_changes(w, "rate")) >= 2 for w in walks)  # (a step changes one thing: every rate step is a rate change with nothing else)
    came_back = 0
    for w in walks:
        seen, prev = {ow.frozen(ow.start())}, ow.frozen(ow.start())
        for s in ow.states(w):
            f = ow.frozen(s)
            came_back += f != prev and f in seen
            seen.add(f)
            prev = f
    assert came_back >= 3


def test_dependent_settings_are_met_with_the_other_one_on_and_off(walks):
    st = [s for w in walks for s in ow.states(w)]
    on = lambda s, n: s[n] != ow.OFF[n]  # noqa: E731
    for dep, needs in (("pause", "trim"), ("limiter", "loudness"), ("peak", "loudness")):
        assert any(on(s, dep) and on(s, needs) for s in st) and any(on(s, dep) and not on(s, needs) for s in st), (dep, needs)


def test_the_pitch_walk_and_the_dither_walk_hold_their_situations(walks):
    on = lambda s, n: s[n] != ow.OFF[n]  # noqa: E731
    steps = lambda w: list(zip(range(len(w)), [ow.start()] + ow.states(w)[:-1], ow.states(w), w))  # noqa: E731
    # walk 5: the shift under the compressor, the de-esser, trimming and loudness
    w5 = steps(walks[5])
    assert all(on(s, n) for _, _, s, _ in w5[4:] for n in ("compressor", "deesser", "trim", "loudness"))
    moved = [i for i, p, s, k in w5 if k[:2] == ("set", "pitch") and on(p, "pitch") and on(s, "pitch") and p["pitch"] != s["pitch"]]
    assert sorted(i % 4 for i in moved) == [0, 2]  # even steps: the compressor's report in front once, the de-esser's once
    for i in moved:  # (each goes to a ratio that shares one term with the one before: the table of the way back is another one)
        (a0, b0), (a1, b1) = (ow.pitch_ratio(x["pitch"]) for x in w5[i][1:3])
        assert (a0 == a1) != (b0 == b1)
    under = [(i, p, k) for i, p, s, k in w5 if on(p, "pitch") and on(s, "pitch")]
    assert any(k[0] == "wav" and i % 2 == 0 for i, p, k in under)
    assert [k[1] for i, p, k in under if k[0] == "batch"] == [2, 1, 0]  # a grow, a shrink and the row count alone (BATCHES), all shifted
    assert {k[1] for _, _, _, k in w5 if k[0] == "op"} == {"time_stretch", "pitch"}
    vals = [k[2] for _, _, _, k in w5 if k[:2] == ("set", "pitch")]
    assert vals[-3] is not None and vals[-2] is None and vals[-1] == vals[-3]
    assert ("refuse", "pitch", 12.5) in walks[5]
    # walk 6: dither beside the rate, loudness and the limiter, each state at a step whose encoded fetches hold a PCM encoding
    w6 = [(i, p, s, k) for i, p, s, k in steps(walks[6]) if {"pcm16", "pcm24"} & set(ow.encodings(i))]
    assert len(w6) >= 12
    assert any(on(s, "dither") and on(s, "rate") and not any(on(s, n) for n in ow.SETTINGS if n not in ("dither", "rate", "limiter")) for _, _, s, _ in w6)
    assert any(on(s, "dither") and on(s, "loudness") and on(s, "limiter") for _, _, s, _ in w6)
    assert any(on(s, "dither") and not on(s, "rate") for _, _, s, _ in w6)
    assert any(i % 2 == 0 and k[:2] == ("set", "dither") and {p["dither"], s["dither"]} == set(ow.VALUES["dither"][:2]) for i, p, s, k in w6)
    assert ("refuse", "dither", (4, 7)) in walks[6] and {k[1] for k in walks[6] if k[0] == "op"} == {"loudness_range", "encode_ex"}


# ---- sensitivity: a fake engine with the real one's keys ------------------------------------------------------------------------------------
KEYS = dict(
    ed=("seq", "hz", "db", "keep", "fade", "Wo", "buf", "mp", "fl", "cp", "ds", "ps"),   # EdKey
    cp=("seq", "hz", "fl", "cp", "Wo", "buf", "ds", "ps"),                               # CpKey
    ds=("seq", "hz", "fl", "ds", "Wo", "buf", "ps"),                                     # DsKey
    ps=("seq", "gen", "W", "B", "buf"),                                                  # PsKey
    ps_rs=("a", "b"),                                                                    # ps_rs_: the table of the way back, per ratio
    st_win=("hz", "ms"), lm_win=("hz", "ms"),                                      # st_window, lm_window
    lo_n=("n", "base", "rows", "W"), cp_n=("n", "base", "rows", "W"), ds_n=("n", "base", "rows", "W"), fl_n=("base", "rows", "W"),
)
OMISSIONS = [(c, f) for c, fs in KEYS.items() for f in fs if f not in ("n", "base")]
IMPLIED = ({(c, f) for c in ("ed", "cp", "ds") for f in ("hz", "Wo", "buf")}
           | {(c, f) for c in ("lo_n", "cp_n", "ds_n") for f in ("rows", "W")}
           | {("ps", f) for f in ("W", "B", "buf")})


def _h(*parts):
    return hashlib.sha1(repr(parts).encode()).hexdigest()[:12]


class Fake:
    """The output stage as far as its kept state goes.  Every kept thing has a truth (a hash of what it really depends on) and is looked
    up under a key; a key that matches hands back what was kept.  omit = (cache, field) leaves one field out of one key.  `harmless`
    counts the matches of a shortened key and how many of them the whole key would not have matched."""

    def __init__(self, omit=None):
        self.omit, self.s, self.seq = omit, ow.start(), 1
        self.gen = dict(filters=0, compressor=0, deesser=0, pitch=0)  # (fl_gen_, cp_gen_, ds_gen_, ps_gen_: bumped by every set step)
        self.kept, self.cap, self.base = {}, {}, {}
        self.short_hits = self.wrong_hits = 0

    # -- geometry
    def native(self):
        """(rows, W) at the model's rate: what the shift works on"""
        lens, durs, _ = ow.BATCHES[self.s["batch"]]
        return len(lens), math.ceil(max(durs) / ow.SPEED * ow.NATIVE_HZ / 3072) * 3072

    def dims(self):
        B, W = self.native()
        hz = ow.rate_of(self.s)
        return B, hz, -(-W * hz // ow.NATIVE_HZ)

    def buf(self, name, need):
        if need > self.cap.get(name, 0):
            self.cap[name] = need + need // 4
            self.base[name] = self.base.get(name, 0) + 1
        return self.base[name]

    # -- the kept state
    def lookup(self, cache, key, truth, refill=False):
        """what is kept under the key, or (a miss, or refill: the path computes anyway) the truth, kept from now on"""
        full = tuple(key[f] for f in KEYS[cache])
        short = tuple(key[f] for f in KEYS[cache] if (cache, f) != self.omit)
        had = self.kept.get(cache)
        if had and not refill and had[0] == short:
            if self.omit and self.omit[0] == cache:
                self.short_hits += 1
                self.wrong_hits += had[1] != full
            return had[2]
        self.kept[cache] = (short, full, truth)
        return truth

    def play(self, step):
        if step[0] == "set":
            if step[1] in self.gen:
                self.gen[step[1]] += 1
            self.s = ow.apply(self.s, step)
        elif step[0] in ("batch", "wav"):
            self.s = ow.apply(self.s, step)
            self.seq += 1  # (batch_run bumps ed_seq_ and nothing else: the keys alone tell its batch from the one before)
            if step[0] == "wav":
                self.kept.pop("ed", None)
        elif step[0] == "op":
            if step[1] in ("loudness", "join"):
                self.kept.pop("lo_n", None)  # (lo_n_.clear() in lo_op and op_join)
        elif step[0] == "fetch":
            self.output({"enc": "enc0", "join_programme": "join_programme", "join_row": "join_row"}.get(step[1], step[1]), 0)

    # -- the stages
    def on(self, name):
        return self.s[name] != ow.OFF[name]

    def chain_key(self):
        B, hz, Wo = self.dims()
        return dict(seq=self.seq, hz=hz, Wo=Wo, fl=self.gen["filters"], cp=self.gen["compressor"], ds=self.gen["deesser"], ps=self.gen["pitch"])

    def shifted(self):
        """ps_batch: the rows at the model's rate behind the shift, kept per batch and setting; the table of the way back is looked up
        only when the rows are not kept"""
        B, W = self.native()
        a, b = ow.pitch_ratio(self.s["pitch"])
        key = dict(seq=self.seq, gen=self.gen["pitch"], W=W, B=B, buf=self.buf("ps", B * (W + -(-W * a // b))))
        had = self.kept.get("ps")
        if had and had[0] == tuple(key[f] for f in KEYS["ps"] if ("ps", f) != self.omit):
            return self.lookup("ps", key, None)
        taps = self.lookup("ps_rs", dict(a=a, b=b), _h("taps", a, b))
        return self.lookup("ps", key, _h("shifted", self.s["batch"], self.s["wav"], a, taps))

    def source(self):
        """out_source: the rows (with pitch on the shifted ones) behind resampler, chain, de-esser and compressor; the two reports' maxima
        are kept on the way"""
        B, hz, Wo = self.dims()
        s, k = self.s, self.chain_key()
        x = _h("src", s["batch"], s["wav"], hz, self.shifted() if self.on("pitch") else None)
        spans = _h("spans", s["batch"], hz)
        if self.on("filters"):
            n = self.lookup("fl_n", dict(base=self.buf("fl", B * Wo), rows=B, W=Wo), (B, Wo))
            x = _h(x, s["filters"], n)
        if self.on("deesser"):
            base = self.buf("ds", B * Wo)
            n = self.lookup("ds_n", dict(n=spans, base=base, rows=B, W=Wo), spans)
            x = _h(x, s["deesser"])
            self.lookup("ds", dict(k, buf=base), _h("dsmax", x, n), refill=True)
        if self.on("compressor"):
            base = self.buf("cp", B * Wo)
            n = self.lookup("cp_n", dict(n=spans, base=base, rows=B, W=Wo), spans)
            x = _h(x, s["compressor"])
            self.lookup("cp", dict(k, buf=base), _h("cpmax", x, n), refill=True)
        return x

    def edges(self, pauses):
        B, hz, Wo = self.dims()
        db, keep, fade = self.s["trim"] or (40.0, 20.0, 5.0)
        mp = (self.s["pause"] or 300.0) if pauses else 0.0
        base = self.buf("ed", B * Wo * (2 if pauses else 1))
        key = dict(self.chain_key(), db=db, keep=keep, fade=fade, mp=mp, buf=base)
        had = self.kept.get("ed")
        short = tuple(key[f] for f in KEYS["ed"] if ("ed", f) != self.omit)
        if had and had[0] == short:
            return self.lookup("ed", key, None)
        return self.lookup("ed", key, _h("edges", self.source(), hz, db, keep, fade, mp))

    def pause_active(self):
        return self.on("pause") and self.on("trim")

    def measure(self, x, rows, W, n):
        """lo_rows: the spans uploaded unless kept, the rows measured over them"""
        n = self.lookup("lo_n", dict(n=n, base=self.buf("lo", rows * W), rows=rows, W=W), n)
        return _h("lufs", x, n, self.s["loudness"], self.s["peak"], self.on("limiter"))

    def gain_step(self, x, m):
        if not (self.on("limiter") and self.on("loudness")):
            return _h(x, m)
        B, hz, Wo = self.dims()
        win = self.lookup("lm_win", dict(hz=hz, ms=self.s["limiter"]), _h("hann", hz, self.s["limiter"]))
        return _h("limited", x, m, win, self.s["peak"], self.s["loudness"])

    def st_window(self):
        hz = self.dims()[1]
        fade = (self.s["trim"] or (40.0, 20.0, 5.0))[2]
        return self.lookup("st_win", dict(hz=hz, ms=fade), _h("fade", hz, fade))

    def dithered(self, enc, scope):
        """what the store adds to an output's truth: nothing kept, and nothing at all unless the encoding is one dither applies to"""
        return (self.s["dither"], scope) if self.on("dither") and enc in ("pcm16", "pcm24") else None

    def rows_out(self, enc):
        enc = (enc, self.dithered(enc, "row"))
        B, hz, Wo = self.dims()
        spans = _h("spans", self.s["batch"], hz)
        if self.on("trim"):
            x = self.source()
            e = self.edges(self.pause_active())
            m = self.measure(x, B, Wo, spans) if self.on("loudness") else None
            return _h("trimmed", self.gain_step(x, m), e, self.st_window(), enc)
        if self.on("loudness"):
            x = self.source()
            return _h("gained", self.gain_step(x, self.measure(x, B, Wo, spans)), enc)
        return _h("plain", self.source(), enc)

    def plan(self):
        """batch_join_plan: from the edges with trimming on"""
        B, hz, Wo = self.dims()
        e = self.edges(self.pause_active()) if self.on("trim") else None
        return _h("plan", self.s["batch"], hz, e), 2, Wo * 3

    def joined(self, scope, measure_only=False):
        B, hz, Wo = self.dims()
        p, G, Wj = self.plan()
        if measure_only or (self.on("loudness") and scope == "programme"):
            x = self.source()
            j = _h("joined", x, p, self.st_window() if self.on("trim") else None)
            m = self.measure(j, G, Wj, _h("prog spans", p))
            return m if measure_only else _h("prog", self.gain_step(j, m))
        x = self.source()
        m = self.measure(x, B, Wo, _h("spans", self.s["batch"], hz)) if self.on("loudness") else None
        return _h("join", self.gain_step(x, m), p, self.st_window() if self.on("trim") else None)

    def output(self, name, i):
        B, hz, Wo = self.dims()
        spans = _h("spans", self.s["batch"], hz)
        if name in ("f32", "slot", "copy"):
            return self.rows_out(name)
        if name in ("enc0", "enc1"):
            return self.rows_out(ow.encodings(i)[int(name[-1])])
        if name == "join_programme":
            return self.joined("programme")
        if name == "join_row":  # (the one joined fetch taken in an encoding: the stream is the programme's)
            return _h(self.joined("row"), self.dithered(ow.encodings(i)[0], "programme"))
        if name == "join_loudness":
            return self.joined("programme", measure_only=True)
        if name == "join_loudness_range":
            return _h("range", self.joined("programme", measure_only=True))
        if name == "loudness":
            return self.measure(self.source(), B, Wo, spans)
        if name == "loudness_range":  # (batch_loudness_range: lo_batch over the same spans, then the report from its partial sums)
            return _h("range", self.measure(self.source(), B, Wo, spans))
        if name == "limiter":
            if not (self.on("limiter") and self.on("loudness")):
                return 0
            x = self.source()
            return self.gain_step(x, self.measure(x, B, Wo, spans))
        if name == "true_peak":
            x = self.source()
            return _h("tp", x, self.gain_step(x, self.measure(x, B, Wo, spans)) if self.on("loudness") else None)
        if name == "silence_edges":
            return self.edges(self.pause_active())
        if name == "pauses":
            return self.edges(True)
        if name in ("compressor", "deesser"):
            if not self.on(name):
                return 0
            c = {"compressor": "cp", "deesser": "ds"}[name]
            k = dict(self.chain_key(), buf=self.buf(c, B * Wo))
            had = self.kept.get(c)
            if not (had and had[0] == tuple(k[f] for f in KEYS[c] if (c, f) != self.omit)):
                self.source()
            return self.lookup(c, k, None)
        raise KeyError(name)

    def take(self, i):
        return {name: self.output(name, i) for name in ow.take_order(i)}


def _fresh(state, i):
    f = Fake()
    f.s = dict(state)
    return f.take(i)


def _caught(walks, omit, every=1):
    """(the first (walk, step, outputs) at which a fake with the omission delivers something else than a fresh fake, or None;
    matches of the shortened key; those the whole key would have refused)"""
    first, short, wrong = None, 0, 0
    for w, walk in enumerate(walks):
        live = Fake(omit)
        for i, step in enumerate(walk):
            live.play(step)
            if (i + 1) % every == 0 or i == len(walk) - 1:
                got, want = live.take(i), _fresh(live.s, i)
                bad = [k for k in want if got[k] != want[k]]
                if bad and first is None:
                    first = (w, i, bad)
        short += live.short_hits
        wrong += live.wrong_hits
    return first, short, wrong


def test_the_fake_with_whole_keys_is_a_fresh_fake_at_every_step(walks):
    assert _caught(walks, None)[0] is None


def test_the_fake_reuses_what_it_keeps(walks):
    """(the sensitivity below would be empty if the fake's caches never hit)"""
    for c in KEYS:
        first, short, wrong = _caught(walks, (c, "no such field"))
        assert first is None and short > 0 and wrong == 0, c


@pytest.mark.parametrize("cache,field", [o for o in OMISSIONS if o not in IMPLIED], ids=lambda v: str(v))
def test_every_omitted_key_field_is_caught_by_a_walk(walks, cache, field):
    first, short, wrong = _caught(walks, (cache, field))
    assert first is not None and wrong > 0, (cache, field, short, wrong)


@pytest.mark.parametrize("cache,field", sorted(IMPLIED), ids=lambda v: str(v))
def test_a_field_the_rest_of_its_key_implies_cannot_be_caught_and_its_omission_is_harmless(walks, cache, field):
    """(module docstring) over every walk the shortened key matches often, and never where the whole key would not have"""
    first, short, wrong = _caught(walks, (cache, field))
    assert first is None and short > 0 and wrong == 0, (cache, field, first, short, wrong)
