"""Tokenizer-side helpers: suppressed-token sets and token → text decoding.

Mirrors faster-whisper 1.2.1 ``get_suppressed_tokens`` and ``Tokenizer`` (upstream,
not vendored).  ``suppress_tokens=[-1]`` expands to the tokenizer's
``non_speech_tokens`` plus ``[transcribe, translate, sot, sot_prev, sot_lm]``.

When a model directory provides ``tokenizer.json`` the non-speech set is computed
from it exactly as upstream does (symbols and their space-prefixed forms encoded
to single tokens).  Without one, the multilingual Whisper table below is used —
it is the text-token part of the published ``suppress_tokens`` list of the
multilingual checkpoints' generation config (parity unpinned: there is no
tokenizer in this image to recompute it).  The English-only vocabulary (51864 ids)
numbers its text tokens differently, so without a ``tokenizer.json`` it has no
non-speech set at all (a warning is logged once) rather than a wrong one.
"""
from __future__ import annotations

import logging
import os
import string
import zlib

from .dims import LANGUAGE_CODES, SpecialTokens

NON_SPEECH_TOKENS_MULTILINGUAL = (
    1, 2, 7, 8, 9, 10, 14, 25, 26, 27, 28, 29, 31, 58, 59, 60, 61, 62, 63, 90, 91, 92, 93, 359,
    503, 522, 542, 873, 893, 902, 918, 922, 931, 1350, 1853, 1982, 2460, 2627, 3246, 3253, 3268,
    3536, 3846, 3961, 4183, 4667, 6585, 6647, 7273, 9061, 9383, 10428, 10929, 11938, 12033, 12331,
    12562, 13793, 14157, 14635, 15265, 15618, 16553, 16604, 18362, 18956, 20075, 21675, 22520,
    26130, 26161, 26435, 28279, 29464, 31650, 32302, 32470, 36865, 42863, 47425, 49870, 50254,
)

_SYMBOLS = list('"#()*+/:;<=>@[\\]^_`{|}~「」『』')
_SYMBOLS += "<< >> <<< >>> -- --- -( -[ (' (\" (( )) ((( ))) [[ ]] {{ }} ♪♪ ♪♪♪".split()
_MISC = set("♩♪♫♬♭♮♯")
UNSPACED_LANGUAGES = frozenset({"zh", "ja", "th", "lo", "my", "yue"})


_BYTE_DECODER: dict = {}
log = logging.getLogger(__name__)
_warned_no_table = False


def _byte_decoder() -> dict:
    """Byte-level BPE's printable stand-in character -> byte (the GPT-2 ``bytes_to_unicode``
    table inverted): printable Latin-1 bytes stand for themselves, the other 68 take the code
    points from 256 up in byte order."""
    if not _BYTE_DECODER:
        keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
        n = 0
        for b in range(256):
            if b in keep:
                _BYTE_DECODER[chr(b)] = b
            else:
                _BYTE_DECODER[chr(256 + n)] = b
                n += 1
    return _BYTE_DECODER


class WhisperTokenizer:
    """Thin wrapper; text decoding needs a ``tokenizer.json`` (``tokenizers`` package)."""

    def __init__(self, n_vocab: int, tokenizer_json: str | None = None):
        self.special = SpecialTokens.for_vocab(n_vocab)
        self.n_vocab = n_vocab
        self._tok = None
        if tokenizer_json and os.path.exists(tokenizer_json):
            from tokenizers import Tokenizer  # available in the image

            self._tok = Tokenizer.from_file(tokenizer_json)

    @property
    def has_text(self) -> bool:
        return self._tok is not None

    def encode(self, text: str) -> list[int]:
        if self._tok is None:
            return []
        return self._tok.encode(text, add_special_tokens=False).ids

    def decode(self, tokens) -> str:
        text_tokens = [int(t) for t in tokens if int(t) < self.special.eot]
        if self._tok is None:
            return "".join(f"<|{t}|>" for t in text_tokens)
        return self._tok.decode(text_tokens, skip_special_tokens=False)

    def token_bytes(self, token: int) -> bytes:
        """The UTF-8 bytes one token stands for (a token may hold part of a character, so the
        bytes of consecutive tokens concatenate to the text's; OpenAI's logprobs ``bytes``).
        Without a ``tokenizer.json``: the bytes of ``decode``'s ``<|id|>`` stand-in."""
        t = int(token)
        if self._tok is None:
            return f"<|{t}|>".encode()
        piece = self._tok.id_to_token(t)
        if piece is None:
            return b""
        table = _byte_decoder()
        if all(ch in table for ch in piece):      # byte-level BPE piece
            return bytes(table[ch] for ch in piece)
        return piece.encode("utf-8")              # an added (special) token: its literal text

    def _decode_with_specials(self, tokens) -> str:
        """Text tokens decoded; <|endoftext|> kept as its own marker (it closes the word
        list of ``split_to_word_tokens``); other ids above it dropped."""
        out, run = [], []
        for t in tokens:
            t = int(t)
            if t < self.special.eot:
                run.append(t)
                continue
            if run:
                out.append(self.decode(run))
                run = []
            if t == self.special.eot:
                out.append("<|endoftext|>")
        if run:
            out.append(self.decode(run))
        return "".join(out)

    def split_tokens_on_unicode(self, tokens):
        """faster-whisper ``Tokenizer.split_tokens_on_unicode`` [upstream]: a word closes
        where the tokens so far decode to complete UTF-8 (no U+FFFD that the full text
        does not have at the same place)."""
        full = self._decode_with_specials(tokens)
        rep = "\ufffd"
        words, word_tokens, cur, offset = [], [], [], 0
        for t in tokens:
            cur.append(int(t))
            dec = self._decode_with_specials(cur)
            at = dec.find(rep)
            if at < 0 or (at + offset < len(full) and full[at + offset] == rep):
                words.append(dec)
                word_tokens.append(cur)
                cur = []
                offset += len(dec)
        return words, word_tokens

    def split_tokens_on_spaces(self, tokens):
        """faster-whisper ``Tokenizer.split_tokens_on_spaces`` [upstream]: sub-words join the
        word before them unless they start with a space, are punctuation or are special."""
        words, word_tokens = [], []
        for sub, sub_tokens in zip(*self.split_tokens_on_unicode(tokens)):
            special = sub_tokens[0] >= self.special.eot
            if special or sub.startswith(" ") or sub.strip() in string.punctuation or not words:
                words.append(sub)
                word_tokens.append(list(sub_tokens))
            else:
                words[-1] += sub
                word_tokens[-1].extend(sub_tokens)
        return words, word_tokens

    def split_to_word_tokens(self, tokens, language: str | None = None):
        """(words, tokens of each word) of ``tokens`` (text ids, usually closed by
        <|endoftext|>, which becomes the last pseudo-word): faster-whisper
        ``Tokenizer.split_to_word_tokens`` [upstream].  Languages written without spaces
        split at Unicode boundaries, the rest at spaces with punctuation kept apart."""
        if language in UNSPACED_LANGUAGES:
            return self.split_tokens_on_unicode(tokens)
        return self.split_tokens_on_spaces(tokens)

    def non_speech_tokens(self) -> tuple:
        if self._tok is None:
            if not self.special.multilingual:
                global _warned_no_table
                if not _warned_no_table:
                    _warned_no_table = True
                    log.warning("English-only vocabulary without a tokenizer.json: suppress_tokens -1 expands to "
                                "the special tokens only (no non-speech symbol table for this vocabulary)")
                return ()
            return NON_SPEECH_TOKENS_MULTILINGUAL
        result = {self.encode(" -")[0], self.encode(" '")[0]}
        for symbol in _SYMBOLS + list(_MISC):
            for tokens in (self.encode(symbol), self.encode(" " + symbol)):
                if len(tokens) == 1 or symbol in _MISC:
                    result.add(tokens[0])
        return tuple(sorted(result))

    def language_code(self, lang_token: int) -> str:
        if not self.special.multilingual:
            return "en"
        i = lang_token - self.special.first_lang
        return LANGUAGE_CODES[i] if 0 <= i < len(LANGUAGE_CODES) else "en"

    def language_token(self, code: str) -> int | None:
        if not self.special.multilingual:
            return None  # an English-only start sequence has no language token
        try:
            i = LANGUAGE_CODES.index(code)
        except ValueError as e:
            raise ValueError(f"unsupported language: {code!r}") from e
        if i >= self.special.n_langs:
            raise ValueError(f"language {code!r} not in this vocabulary")
        return self.special.first_lang + i


def get_suppressed_tokens(tok: WhisperTokenizer, suppress_tokens=(-1,)) -> tuple:
    st = tok.special
    s = list(suppress_tokens or [])
    if -1 in s:
        s = [t for t in s if t >= 0]
        s.extend(tok.non_speech_tokens())
    s.extend([st.transcribe, st.translate, st.sot, st.sot_prev, st.sot_lm])
    return tuple(sorted(set(s)))


def compression_ratio(text: str) -> float:
    b = text.encode("utf-8")
    return len(b) / len(zlib.compress(b)) if b else 0.0
