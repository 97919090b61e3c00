"""Whisper's language handling on the host (no GPU): the language tables, the tokenizer's language tokens and
``with_language``, language and task in the initial tokens, ``transcribe()`` / ``transcribe_many()`` on a multilingual stub with
``detect_language`` and ``decode`` scripted, ``decode_many``'s per-window fields, and the ABI of ``hirest_whisper_language_tail``."""
import dataclasses
import os
import re
import types

import pytest
import torch

import _whisper_lang as L
from hirest_amd import _lib, synth, whisper

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- tables
def test_language_tables_are_whispers():
    tw = pytest.importorskip("transformers").models.whisper.tokenization_whisper
    assert whisper.LANGUAGES == tw.LANGUAGES and list(whisper.LANGUAGES) == list(tw.LANGUAGES)        # the order is the tokens' order
    assert whisper.TO_LANGUAGE_CODE == tw.TO_LANGUAGE_CODE
    assert len(whisper.LANGUAGES) == 100 and whisper.LANGUAGES["yue"] == "cantonese"


def test_language_code_resolution():
    f = whisper.language_code
    assert f("en") == f("EN") == f("English") == f("english ") == "en"
    assert f("castilian") == f("Spanish") == f("es") == "es" and f("Mandarin") == "zh" and f("haw") == "haw" and f("Cantonese") == "yue"
    assert f("moldovan") == f("Moldavian") == f("romanian") == "ro"
    for bad in ("klingon", "", "e", "auto", None, 5):
        with pytest.raises(ValueError, match=re.escape(repr(bad))):
            f(bad)


# ---------------------------------------------------------------------------------------------------------------- tokenizer
def _wide_specials(n_languages):
    """small.en's layout at the real size with ``n_languages`` language slots after sot, given in REVERSE id order (the table does not
    rely on the order of the dict), plus two look-alikes that are no languages"""
    eot = 50256
    codes = list(whisper.LANGUAGES)[:n_languages]
    sp = {"<|endoftext|>": eot, "<|startoftranscript|>": eot + 1}
    sp.update({f"<|{c}|>": eot + 2 + i for i, c in reversed(list(enumerate(codes)))})
    base = eot + 2 + n_languages
    sp.update({"<|translate|>": base, "<|transcribe|>": base + 1, "<|startoflm|>": base + 2, "<|startofprev|>": base + 3, "<|nospeech|>": base + 4,
               "<|notimestamps|>": base + 5, "<|zz|>": base + 6, "<|english|>": base + 7})
    return sp, codes


@pytest.fixture(scope="module")
def wide_vocab():
    return synth.whisper_vocab(50256)


@pytest.mark.parametrize("n", [99, 100])
def test_language_tokens_of_the_released_vocabularies(n, wide_vocab):
    sp, codes = _wide_specials(n)
    tok = whisper.Tokenizer(*wide_vocab, sp, language="en", task="transcribe")
    ids = tok.all_language_tokens
    assert len(ids) == n and list(ids) == sorted(ids) == list(range(50258, 50258 + n))
    assert list(tok.all_language_codes) == codes and ("yue" in tok.all_language_codes) == (n == 100)
    assert all(sp[f"<|{c}|>"] == i for i, c in zip(ids, tok.all_language_codes))                      # aligned
    assert tok.language_token == 50258 and tok.to_language_token("de") == 50260
    assert tok.sot_sequence == (50257, 50258, sp["<|transcribe|>"])
    assert tok.timestamp_begin == sp["<|notimestamps|>"] + 1


def test_language_tokens_of_the_synthetic_vocabulary():
    tok = L.tokenizer(100)
    assert tok.all_language_tokens == (102, 103, 104, 105) and tok.all_language_codes == L.LANGS
    assert tok.language_token == 102 and tok.sot_sequence == (101, 102, 107)
    plain = synth.whisper_tokenizer(100)                                                              # English-only: none
    assert plain.all_language_tokens == () and plain.all_language_codes == () and plain.sot_sequence == (101,)
    with pytest.raises(ValueError):
        plain.language_token
    with pytest.raises(KeyError):
        tok.to_language_token("fr")


def test_with_language_is_a_copy():
    tok = L.tokenizer(100)
    ns = tok.non_speech_tokens
    de = tok.with_language("German", "translate")
    assert (de.language, de.task) == ("de", "translate") and (tok.language, tok.task) == ("en", "transcribe")
    assert de.sot_sequence == (101, 104, 106) and tok.sot_sequence == (101, 102, 107)
    assert de.bpe is tok.bpe and de.specials is tok.specials and de.non_speech_tokens is ns            # nothing is rebuilt
    assert de.all_language_tokens == tok.all_language_tokens and de.encode(" the") == tok.encode(" the")
    undetermined = tok.with_language(None, "transcribe")
    assert undetermined.language is None and undetermined.sot_sequence == (101, 107) and tok.language == "en"
    with pytest.raises(ValueError):
        tok.with_language("klingon")
    with pytest.raises(ValueError):
        tok.with_language("fr")                                                                       # a language, but not of this vocabulary
    with pytest.raises(ValueError):
        tok.with_language("de", "lang_id")


# ---------------------------------------------------------------------------------------------------------------- initial tokens
def test_initial_tokens_language_and_task():
    tok, f, O = L.tokenizer(100), whisper._initial_tokens, whisper.DecodingOptions
    sot, en, zh, de, es, translate, transcribe = 101, 102, 103, 104, 105, 106, 107
    assert f(tok, O(), 48) == ([sot, en, transcribe], 0)                                              # the tokenizer's own
    assert f(tok, O(language="de"), 48) == ([sot, de, transcribe], 0)
    assert f(tok, O(language="Castilian", task="translate"), 48) == ([sot, es, translate], 0)
    assert f(tok, O(task="translate"), 48) == ([sot, en, translate], 0)
    assert f(tok, O(language="ZH", without_timestamps=True), 48) == ([sot, zh, transcribe, tok.no_timestamps], 0)
    got, sot_index = f(tok, O(language="de", task="translate", prompt=[1, 2, 3]), 48)
    assert got == [tok.sot_prev, 1, 2, 3, sot, de, translate] and sot_index == 4
    # what with_language() set is the default of what the options leave open
    assert f(tok.with_language("de", "translate"), O(), 48) == ([sot, de, translate], 0)
    assert f(tok.with_language("de", "translate"), O(language="es"), 48) == ([sot, es, translate], 0)
    # a detected language (decode() passes it) goes where the options and the tokenizer name none
    none = tok.with_language(None, "transcribe")
    assert f(none, O(), 48, "zh") == ([sot, zh, transcribe], 0)
    with pytest.raises(ValueError, match="no language"):
        f(none, O(), 48)
    with pytest.raises(ValueError):
        f(tok, O(language="klingon"), 48)
    with pytest.raises(ValueError):
        f(tok, O(language="fr"), 48)
    with pytest.raises(NotImplementedError):
        f(tok, O(task="lang_id"), 48)


def test_initial_tokens_of_an_english_only_tokenizer_ignore_both():
    tok, f, O = synth.whisper_tokenizer(100), whisper._initial_tokens, whisper.DecodingOptions
    for o in (O(), O(language="de"), O(task="translate"), O(language="German", task="translate"), O(language="klingon")):
        assert f(tok, o, 48) == ([tok.sot], 0)
    assert f(tok, O(language="de", task="translate", prompt=[4, 5]), 48) == ([tok.sot_prev, 4, 5, tok.sot], 3)
    r = whisper.DecodingResult()
    assert r.language == "en" and r.language_probs is None


def test_an_english_only_checkpoint_with_language_tokens_in_its_vocabulary(monkeypatch, wide_vocab):
    """The released ``*.en`` vocabularies carry the 99 language tokens too (ids 50258 .. 50356, where synth leaves the slots free).
    load_model gives such a model language=None, task=None: English-only by configuration.  Nothing of the language handling may
    reach it: the prompt stays [sot], nothing is detected, transcribe() says "en"."""
    sp = synth.whisper_special_tokens(50256)
    sp.update({f"<|{c}|>": 50258 + i for i, c in enumerate(list(whisper.LANGUAGES)[:99])})
    tok = whisper.Tokenizer(*wide_vocab, sp, language=None, task=None)                                # what load_model builds for small.en
    assert len(tok.all_language_tokens) == 99 and not tok.multilingual and tok.sot_sequence == (50257,)
    f, O = whisper._initial_tokens, whisper.DecodingOptions
    for o in (O(), O(language="en"), O(language="English", task="transcribe"), O(language="de", task="translate")):
        assert f(tok, o, 448) == ([tok.sot], 0)
    assert f(tok, O(language="en", prompt=[4, 5]), 448) == ([tok.sot_prev, 4, 5, tok.sot], 3)
    with pytest.raises(ValueError, match="lang id"):                  # (raised before anything touches a device)
        whisper.detect_language(_stub_model(tok), torch.zeros((80, 3000)))
    monkeypatch.setattr(whisper, "detect_language", lambda *a, **k: pytest.fail("an English-only model detects nothing"))
    requests = []
    monkeypatch.setattr(whisper, "decode", lambda model, segment, options: requests.append(options) or _res(tok, _whole(tok)))
    for kw in ({}, {"language": "English", "task": "transcribe"}, {"language": None}):
        out = whisper.transcribe(_stub_model(tok), _mel(0, 3000), temperature=0.0, **kw)
        assert out["language"] == "en" and len(out["segments"]) == 1
    assert [o.language for o in requests] == [None, "English", None]                                  # the options pass through untouched
    # the same vocabulary configured as a multilingual checkpoint's is multilingual; both configurations share the tables
    ml = tok.with_language("en", "transcribe")
    assert ml.multilingual and not tok.multilingual and f(ml, O(), 448) == ([tok.sot, 50258, tok.transcribe], 0)
    assert not ml.with_language(None, None).multilingual and ml.with_language(None).multilingual


# ---------------------------------------------------------------------------------------------------------------- transcribe on a stub
def _stub_model(tok):
    return types.SimpleNamespace(dims={"n_mels": 80, "n_audio_ctx": 1500}, is_multilingual=True, device=torch.device("cpu"), tokenizer=tok)


def _mel(file, frames):
    mel = torch.zeros((80, frames + 3000))
    mel[0] = torch.arange(frames + 3000, dtype=torch.float32)        # row 0: the frame number; row 1: the file
    mel[1] = float(file)
    return mel


def _whole(tok):
    return [tok.timestamp_begin] + tok.encode(" the") + [tok.timestamp_begin + 1500]                  # one segment over the whole window


def _res(tok, tokens):
    return whisper.DecodingResult(tokens=list(tokens), text=tok.decode(tokens), avg_logprob=-0.2, no_speech_prob=0.01, temperature=0.0,
                                  compression_ratio=1.2)


def _scripted_detection(monkeypatch, tok, language_of_file):
    """detect_language replaced: records (file, first frame) of the windows of each call and answers by file"""
    calls = []

    def fake_detect(model, mel, tokenizer=None):
        assert mel.ndim == 3 and tuple(mel.shape[1:]) == (80, 3000) and tokenizer is tok
        calls.append([(int(m[1, 0]), int(m[0, 0])) for m in mel])
        tokens = torch.tensor([tok.to_language_token(language_of_file[int(m[1, 0])]) for m in mel])
        return tokens, [{c: float(c == language_of_file[int(m[1, 0])]) for c in tok.all_language_codes} for m in mel]
    monkeypatch.setattr(whisper, "detect_language", fake_detect)
    return calls


def test_transcribe_detects_once_on_the_first_window(monkeypatch):
    tok = L.tokenizer(100)
    detections = _scripted_detection(monkeypatch, tok, {0: "de"})
    requests = []

    def fake_decode(model, segment, options):
        requests.append((int(segment[0, 0]), options))
        return _res(tok, _whole(tok))
    monkeypatch.setattr(whisper, "decode", fake_decode)
    out = whisper.transcribe(_stub_model(tok), _mel(0, 7000), temperature=0.0, task="translate")
    assert detections == [[(0, 0)]]                                                                   # once, with the first window
    assert [r[0] for r in requests] == [0, 3000, 6000]
    assert all(o.language == "de" and o.task == "translate" for _, o in requests)
    assert out["language"] == "de" and len(out["segments"]) == 3
    # a language that is given is resolved and nothing is detected
    detections.clear(), requests.clear()
    out = whisper.transcribe(_stub_model(tok), _mel(0, 3000), temperature=0.0, language="Castilian")
    assert detections == [] and out["language"] == "es" and [o.language for _, o in requests] == ["es"] and requests[0][1].task == "transcribe"
    with pytest.raises(ValueError, match="klingon"):
        whisper.transcribe(_stub_model(tok), _mel(0, 3000), language="klingon")
    # an English-only tokenizer: "en" whatever is asked, no detection, and the options pass through untouched
    plain = synth.whisper_tokenizer(100)
    requests.clear()
    out = whisper.transcribe(_stub_model(plain), _mel(0, 3000), temperature=0.0)
    assert detections == [] and out["language"] == "en" and requests[0][1].language is None


def test_transcribe_many_detects_the_seated_files_together(monkeypatch):
    tok = L.tokenizer(100)
    languages = {0: "de", 1: "zh", 2: "es", 3: "en"}
    frames = {0: 6000, 1: 3000, 2: 0, 3: 3000}                                                        # file 2 has no content
    detections = _scripted_detection(monkeypatch, tok, languages)
    rounds = []

    def fake_decode_many(model, segments, options):
        rounds.append([(int(s[1, 0]), int(s[0, 0]), o.language) for s, o in zip(segments, options)])
        return [_res(tok, _whole(tok)) for _ in segments]
    monkeypatch.setattr(whisper, "decode_many", fake_decode_many)
    monkeypatch.setattr(whisper, "decode", lambda *a, **k: pytest.fail("transcribe_many decodes through decode_many"))
    out = whisper.transcribe_many(_stub_model(tok), [_mel(i, frames[i]) for i in range(4)], files_in_flight=2, temperature=0.0)
    # one detection call per seating round, over the first windows of the files that took a slot in it; the file without content never
    # takes one, and its result still names the language of its (empty) first window, as Whisper's does
    assert detections == [[(0, 0), (1, 0)], [(2, 0)], [(3, 0)]]
    assert rounds == [[(0, 0, "de"), (1, 0, "zh")], [(0, 3000, "de"), (3, 0, "en")]]
    assert [o["language"] for o in out] == ["de", "zh", "es", "en"]
    assert [len(o["segments"]) for o in out] == [2, 1, 0, 1]


# ---------------------------------------------------------------------------------------------------------------- decode_many's fields
def test_decode_many_takes_a_language_per_window(monkeypatch):
    seen = []
    monkeypatch.setattr(whisper, "_decode_windows", lambda model, mel, opts, rows: (seen.append(opts) or ([None] * len(opts), [None] * len(opts))))
    mels, O = torch.zeros((2, 80, 3000)), whisper.DecodingOptions
    model = _stub_model(L.tokenizer(100))
    whisper.decode_many(model, mels, [O(language="de"), O(language="zh", temperature=0.4, best_of=3, seed=7, prompt=[1])])
    assert [o.language for o in seen[0]] == ["de", "zh"]
    assert "language" in whisper._PER_WINDOW_OPTIONS
    for field, value in (("task", "translate"), ("without_timestamps", True), ("sample_len", 5), ("suppress_blank", False),
                         ("max_initial_timestamp", None), ("suppress_tokens", "5")):
        assert field not in whisper._PER_WINDOW_OPTIONS
        with pytest.raises(ValueError, match=field):
            whisper.decode_many(model, mels, [O(), dataclasses.replace(O(), **{field: value})])
    assert len(seen) == 1


# ---------------------------------------------------------------------------------------------------------------- the entry point
def test_language_tail_entry_declared_bound_and_checked():
    text = open(os.path.join(REPO, "include", "hirest_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    name = "hirest_whisper_language_tail"
    lib = _lib.load()
    assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.hirest_abi_version() == 4                                                              # additive
    f = lib.hirest_whisper_language_tail
    assert f(None, 0, 1, 4, None, 1, None, None, None) == -1
    one = 8                                                          # any non-null address: the checks below return before a launch
    assert f(one, 200, 0, 200, one, 4, one, one, None) == -1 and f(one, 200, 1, 0, one, 4, one, one, None) == -1
    assert f(one, 200, 1, 200, one, 0, one, one, None) == -2 and f(one, 200, 1, 200, one, 129, one, one, None) == -2       # 1 <= L <= 128
    assert f(one, 196, 1, 200, one, 4, one, one, None) == -2                                           # a row stride below the row


def test_language_tail_kernel_does_not_spill(tmp_path):
    from test_code_objects import LIB, kernel_notes
    path = os.path.join(LIB, "whisper_dec.o")
    if not os.path.isfile(path):
        pytest.skip("whisper_dec.o not built (run __graft_entry__.build())")
    notes = {k.replace("void ", "", 1).replace("(anonymous namespace)::", "").split("(")[0]: v for k, v in kernel_notes(path, str(tmp_path)).items()}
    v = notes["whisper_language_tail_kernel"]
    print(v)
    assert v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, v
