# Lab edit (round 6): the replicated partition's beta stage back to the
# rank-total launch + an all-gather of the totals (no gathered norm partials).
p = "tpl_operator.cpp"
s = open(p).read()
old = "if (op->dist->nranks <= kPbRanks && g2max <= kTPB) {"
assert old in s
open(p, "w").write(s.replace(old, "if (false && op->dist->nranks <= kPbRanks && g2max <= kTPB) {"))
