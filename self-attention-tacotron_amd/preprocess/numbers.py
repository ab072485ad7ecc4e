"""Numbers -> words for the English cleaners (the behaviour of reference preprocess/numbers.py, which delegates the wording to the
`inflect` package; written out here).  Rules, in order: commas inside numbers removed; `£N` -> `N pounds`; dollars and cents with
singular / plural units; `a.b` -> `a point b`; ordinals; cardinals, those from 1001 to 2999 read as years.
Where inflect's wording was not verified (DESIGN.md lists the cases) the choice made here is marked UNVERIFIED."""
import re

_ONES = ["zero", "one", "two", "three", "four", "five", "six", "seven", "eight", "nine", "ten", "eleven", "twelve", "thirteen",
         "fourteen", "fifteen", "sixteen", "seventeen", "eighteen", "nineteen"]
_TENS = ["", "", "twenty", "thirty", "forty", "fifty", "sixty", "seventy", "eighty", "ninety"]
_GROUPS = ["", " thousand", " million", " billion", " trillion", " quadrillion", " quintillion", " sextillion", " septillion",
           " octillion", " nonillion", " decillion"]
_ORDINAL = {"one": "first", "two": "second", "three": "third", "five": "fifth", "eight": "eighth", "nine": "ninth",
            "twelve": "twelfth"}


def _below_hundred(n):
    if n < 20:
        return _ONES[n]
    return _TENS[n // 10] + ("-" + _ONES[n % 10] if n % 10 else "")


def _below_thousand(n, andword):
    if n < 100:
        return _below_hundred(n)
    rest = n % 100
    return _ONES[n // 100] + " hundred" + ((" " + andword if andword else "") + " " + _below_hundred(rest) if rest else "")


def cardinal(n, andword=""):
    """`twelve thousand, three hundred forty-five`: groups of three digits joined by `, ` (UNVERIFIED against inflect above 3000:
    the comma), no `and` unless andword is given"""
    if n == 0:
        return _ONES[0]
    groups, i = [], 0
    while n:
        n, g = divmod(n, 1000)
        if g:
            if i >= len(_GROUPS):
                raise ValueError("number too large to spell")
            groups.append(_below_thousand(g, andword) + _GROUPS[i])
        i += 1
    return ", ".join(reversed(groups))


def ordinal(n):
    """`twenty-second`, `one hundred and first` (UNVERIFIED: inflect's default keeps `and` in ordinals, the reference calls it with
    its defaults there)"""
    words = cardinal(n, andword="and")
    head, sep, last = words.rpartition("-") if "-" in words.rsplit(" ", 1)[-1] else words.rpartition(" ")
    if last in _ORDINAL:
        last = _ORDINAL[last]
    elif last.endswith("y"):
        last = last[:-1] + "ieth"
    else:
        last += "th"
    return head + sep + last


def year(n):
    """1001 .. 2999: `two thousand`, `two thousand five`, `eighteen hundred`, else two pairs - `nineteen ninety-nine`, and with a
    leading zero in the second pair `nineteen oh five` (UNVERIFIED: inflect's group=2 wording with zero='oh')"""
    if n == 2000:
        return "two thousand"
    if 2000 < n < 2010:
        return "two thousand " + _below_hundred(n % 100)
    if n % 100 == 0:
        return _below_hundred(n // 100) + " hundred"
    hi, lo = divmod(n, 100)
    return _below_hundred(hi) + " " + ("oh " + _ONES[lo] if lo < 10 else _below_hundred(lo))


def number_words(n):
    return year(n) if 1000 < n < 3000 else cardinal(n)


_comma_number = re.compile(r"[0-9][0-9,]+[0-9]")
_pounds = re.compile(r"£([0-9,]*[0-9]+)")
_dollars = re.compile(r"\$([0-9.,]*[0-9]+)")
_decimal = re.compile(r"([0-9]+)\.([0-9]+)")
_ordinal_re = re.compile(r"([0-9]+)(st|nd|rd|th)")
_number = re.compile(r"[0-9]+")


def _dollar_words(m):
    parts = m.group(1).split(".")
    if len(parts) > 2:
        return m.group(1) + " dollars"
    dollars = int(parts[0]) if parts[0] else 0
    cents = int(parts[1]) if len(parts) > 1 and parts[1] else 0
    said = []
    if dollars:
        said.append("%d %s" % (dollars, "dollar" if dollars == 1 else "dollars"))
    if cents:
        said.append("%d %s" % (cents, "cent" if cents == 1 else "cents"))
    return ", ".join(said) if said else "zero dollars"


def normalize_numbers(text):
    text = _comma_number.sub(lambda m: m.group(0).replace(",", ""), text)
    text = _pounds.sub(r"\1 pounds", text)
    text = _dollars.sub(_dollar_words, text)
    text = _decimal.sub(r"\1 point \2", text)
    text = _ordinal_re.sub(lambda m: ordinal(int(m.group(1))), text)
    return _number.sub(lambda m: number_words(int(m.group(0))), text)
