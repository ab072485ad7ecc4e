"""Characters -> ids (the contract of reference preprocess/text.py:21): 68 symbols in a fixed order, ids from 1, and a 0 - silence -
in front of and behind every sequence."""

symbols = ([chr(c) for c in range(ord("A"), ord("Z") + 1)] + [chr(c) for c in range(ord("a"), ord("z") + 1)] +
           ["!", "'", '"', "(", ")", "[", "]", ",", "-", ".", ":", ";", "?", "`", " "])
_symbol_to_id = {s: i + 1 for i, s in enumerate(symbols)}
_id_to_symbol = {i + 1: s for i, s in enumerate(symbols)}


def text_to_sequence(text, cleaner, key=None):
    """(ids with a 0 at either end, cleaned text); a character outside the table raises a ValueError naming key and character"""
    clean = cleaner(text)
    seq = [0]
    for ch in clean:
        i = _symbol_to_id.get(ch)
        if i is None:
            raise ValueError("%s: character %r (U+%04X) of %r is not in the symbol table" % (key, ch, ord(ch), clean))
        seq.append(i)
    seq.append(0)
    return seq, clean


def sequence_to_text(seq):
    return "".join(_id_to_symbol[i] for i in seq if i != 0)
