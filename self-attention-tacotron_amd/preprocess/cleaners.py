"""Text cleaners (the behaviour of reference preprocess/cleaners.py).
  basic_cleaners:   lowercase, collapse whitespace                                                   (VCTK)
  english_cleaners: ASCII transliteration, lowercase, numbers, abbreviations, collapse whitespace    (LJSpeech)
Transliteration uses `unidecode` when it is installed; without it: NFKD decomposition with the combining marks dropped plus a
small table for curly quotes, dashes and the ellipsis - anything still outside ASCII is left in place, so that text_to_sequence
refuses it by name instead of training on silently altered text.  `£` is kept through either path, for the pounds rule of
numbers.py (known differences)."""
import re
import unicodedata

from .numbers import normalize_numbers

try:
    from unidecode import unidecode as _unidecode
except ImportError:
    _unidecode = None

_whitespace = re.compile(r"\s+")
_PUNCT = {"\u2018": "'", "\u2019": "'", "\u201a": "'", "\u201b": "'", "\u201c": '"', "\u201d": '"', "\u201e": '"',
          "\u2010": "-", "\u2011": "-", "\u2012": "-", "\u2013": "-", "\u2014": "--", "\u2015": "--", "\u2026": "...",
          "\u00ab": "<<", "\u00bb": ">>", "\u00df": "ss", "\u00e6": "ae", "\u00c6": "AE", "\u0153": "oe", "\u0152": "OE",
          "\u00f8": "o", "\u00d8": "O"}
# the reference's table, `misess` included; each is matched case-insensitively at a word boundary with its full stop
_ABBREVIATIONS = [(re.compile(r"\b%s\." % a, re.IGNORECASE), full) for a, full in [
    ("mrs", "misess"), ("mr", "mister"), ("dr", "doctor"), ("st", "saint"), ("co", "company"), ("jr", "junior"), ("maj", "major"),
    ("gen", "general"), ("drs", "doctors"), ("rev", "reverend"), ("lt", "lieutenant"), ("hon", "honorable"), ("sgt", "sergeant"),
    ("capt", "captain"), ("esq", "esquire"), ("ltd", "limited"), ("col", "colonel"), ("ft", "fort")]]


def _ascii_fallback(text):
    out = []
    for ch in text:
        if ord(ch) < 128:
            out.append(ch)
        elif ch in _PUNCT:
            out.append(_PUNCT[ch])
        else:
            base = "".join(c for c in unicodedata.normalize("NFKD", ch) if not unicodedata.combining(c))
            out.append(base if base and all(ord(c) < 128 for c in base) else ch)
    return "".join(out)


def convert_to_ascii(text):
    one = _unidecode if _unidecode is not None else _ascii_fallback
    return "\u00a3".join(one(part) for part in text.split("\u00a3"))


def lowercase(text):
    return text.lower()


def collapse_whitespace(text):
    return _whitespace.sub(" ", text)


def expand_abbreviations(text):
    for pattern, full in _ABBREVIATIONS:
        text = pattern.sub(full, text)
    return text


def expand_numbers(text):
    return normalize_numbers(text)


def basic_cleaners(text):
    return collapse_whitespace(lowercase(text))


def transliteration_cleaners(text):
    return collapse_whitespace(lowercase(convert_to_ascii(text)))


def english_cleaners(text):
    return collapse_whitespace(expand_abbreviations(expand_numbers(lowercase(convert_to_ascii(text)))))
